// gmres_multi.hip -- right-preconditioned restarted GMRES(m) for s right-hand sides at once: s
// independent GMRES(m) recurrences that share A and run in lockstep, one SpMM per Arnoldi step instead of s SpMVs.  X, B
// and every work block are n x s row-major; the basis is m + 1 such blocks with leading dimension s, one stride apart.
// Every kernel is one of gmres.hip's, widened by a column tile the way krylov_multi.hip widens krylov.hip's:
//   dots     stage 1 of (V_i[:, c], W[:, c]), i <= j, of the tile's columns in ONE pass: a workgroup is a cell of
//            KRYLOV_CELL rows and a tile of TILE columns, a lane keeps its eight rows of W's tile in registers and walks
//            the basis blocks; partial[(i * s + c) * cells + cell] has the single dot's bits on the strided column;
//   fold     stage 2, one workgroup PER COLUMN, and its lane 0 takes the scalar step on column c's two blocks
//            (gmres_fold.h: the text gmres.hip runs);
//   project  W <- W - sum h_i V_i ascending with column c's coefficients from its small-matrix block, in the second
//            Gram-Schmidt pass also stage 1 of (w, w);
//   normal   V_{j+1} = W / eta per column and the block the next step multiplies: Z = V_{j+1}, or dinv o V_{j+1};
//   close    one lane a column decides whether the close acts and back-substitutes; combine; [M^-1;] x update;
//   restart  R = B - A X through the SpMM, the test on the true residual, the next cycle's V_0.
//
// The position.  No kernel takes the count of finished columns from the launch: column c reads it from scalar block c.
// The running columns share it by construction (all start at 0 and step together), so a kernel loops to the largest
// count of its tile and predicates per column; the host only counts steps to know where a close and a restart belong.
//
// The freeze, per column.  A tile reads its columns' blocks once (uniform loads) into a mask and per-column counts.  A
// tile whose columns all rest returns at entry; a mixed tile predicates every load and store by the mask, so a frozen
// column of X or V is neither read nor written.  The SpMM and an applied M^-1 run on whole blocks, into work blocks only.
//
// Width of the accesses.  A full tile whose columns all act moves a row's eight doubles as four 16-byte accesses when
// every base and leading dimension of the launch allows (decided on the host, a template flag); anything else goes
// double by double.  Same values, same order, same bits.
//
// Arithmetic.  Contraction is off at file scope, ahead of gmres.h, as in gmres.hip.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <memory>
#include <type_traits>
#include "../../include/sblas_hip.h"

#pragma clang fp contract(off) // file scope, ahead of gmres.h: a * b + c is two roundings in the scalar step and below

#define GMRES_HD __host__ __device__
#include "gmres.h"
#include "gmres_fold.h"
#include "gmres_multi.h"
#include "krylov_fold.h"
#include "krylov_tile.h" // tile_store
#include "unit_row.h"    // tile_ld, tile_st, tile_id
#include "multi_plan.h"  // the plan base: bind, layout, product, the refusals of start, status

using namespace sblas;

namespace {

constexpr int T = TILE;
constexpr int PL = KRYLOV_PER_LANE;
constexpr unsigned FULL_MASK = (1u << T) - 1u;

// how a column kernel learns column c's count of basis blocks
enum { MODE_FREE = 0,   // from the launch, for every column whose status (when blocks are given) is RUNNING
       MODE_FIRST = 1,  // a step's first kernels: columns + 1 while RUNNING with the cycle not full, else nothing
       MODE_ACTIVE = 2, // behind a step's first fold: columns + 1 while GS_ACTIVE
       MODE_CLOSE = 3 };// behind a close's first kernel: columns while GS_CLOSE

struct MColArgs {
    int64_t n, cells, ldv, vstride, ldw, ldc;
    int s, nk, mode;
    const double *V;    // block i at V + i * vstride, leading dimension ldv
    const double *coef; // column c's coefficients at coef + c * ldc (project: h; combine: y)
    double *w;          // leading dimension ldw.  dots: read; project: updated; combine: written
    double *part;       // dots: partial[(i * s + c) * cells + cell]; project: stage 1 of (w, w), or NULL
    const double *blk;  // s scalar blocks, or NULL (MODE_FREE: every column acts)
};

__device__ __forceinline__ int column_count(const double *blk, int c, int mode, int nk)
{
    if (mode == MODE_FREE && !blk) return nk;
    const long long *ib = reinterpret_cast<const long long *>(blk) + (size_t)c * GMRES_BLOCK_SLOTS; // block-uniform loads, read once
    if (mode == MODE_FREE) return ib[GS_STATUS] == GMRES_RUNNING ? nk : 0;
    if (mode == MODE_FIRST) return ib[GS_STATUS] == GMRES_RUNNING && ib[GS_COLS] < ib[GS_M] ? (int)ib[GS_COLS] + 1 : 0;
    if (mode == MODE_ACTIVE) return ib[GS_ACTIVE] ? (int)ib[GS_COLS] + 1 : 0;
    return ib[GS_CLOSE] ? (int)ib[GS_COLS] : 0;
}

// a workgroup's cell and tile, and what its columns ask for: nk[c] basis blocks of column j0 + c (0: the column rests)
struct TileCols {
    int64_t cell;
    int j0, nmax;
    unsigned mask;
    int nk[T];
    __device__ __forceinline__ TileCols(const MColArgs &a)
    {
        const TileId id = tile_id(a.cells, tiles(a.s));
        cell = id.block, j0 = (int)id.tile * T, nmax = 0, mask = 0;
        const int w = a.s - j0 < T ? a.s - j0 : T;
#pragma unroll
        for (int c = 0; c < T; ++c) {
            nk[c] = c < w ? column_count(a.blk, j0 + c, a.mode, a.nk) : 0;
            if (nk[c] > 0) mask |= 1u << c;
            nmax = nk[c] > nmax ? nk[c] : nmax;
        }
    }
};

// lane t's eight rows of a cell: row k is first + k * KRYLOV_LANES, and exists below n
struct Rows {
    int64_t first, n;
    bool full;
    __device__ __forceinline__ Rows(int64_t cell, int64_t n_) : first(cell * KRYLOV_CELL + threadIdx.x), n(n_), full((cell + 1) * KRYLOV_CELL <= n_) {}
    __device__ __forceinline__ int64_t row(int k) const { return first + (int64_t)k * KRYLOV_LANES; }
    __device__ __forceinline__ bool live(int k) const { return full || row(k) < n; }
};

template <bool F> __device__ __forceinline__ void load_rows(const Rows &r, const double *p, int64_t ld, unsigned mask, double (&v)[PL][T])
{
#pragma unroll
    for (int k = 0; k < PL; ++k) {
        if (r.live(k)) {
            tile_ld<T, F>(p + r.row(k) * ld, mask, v[k]);
        } else {
#pragma unroll
            for (int c = 0; c < T; ++c) v[k][c] = 0.0;
        }
    }
}

template <bool F> __device__ __forceinline__ void store_rows(const Rows &r, double *p, int64_t ld, unsigned mask, const double (&v)[PL][T])
{
#pragma unroll
    for (int k = 0; k < PL; ++k)
        if (r.live(k)) tile_st<T, F>(p + r.row(k) * ld, mask, v[k]);
}

// ---- the multi-dot, stage 1 ------------------------------------------------------------------------------------------
// Column c's lane sum over the lane's rows in order, the product rounded and then the sum, from +0; the butterfly inside
// the wave; the four waves' sums wait in LDS for the one barrier at the end.  Exactly krylov_dot_kernel's order on the
// strided column.  W's tile stays in registers (128 of them) beside ONE basis block's rows in flight: more blocks in
// flight would pass the 256 registers of two workgroups a compute unit, and a column's sum never meets another's.
template <bool WIDE> __global__ __launch_bounds__(KRYLOV_LANES) void gmres_multi_dots_kernel(const MColArgs a)
{
    __shared__ double ws[GMRES_MAX_DOTS][T][4];
    const TileCols tc(a);
    if (tc.mask == 0) return; // every column of the tile rests
    const Rows rows(tc.cell, a.n);
    auto body = [&](auto fast) {
        constexpr bool F = decltype(fast)::value;
        double wv[PL][T];
        load_rows<F>(rows, a.w + tc.j0, a.ldw, tc.mask, wv);
        for (int i = 0; i < tc.nmax; ++i) {
            const double *vb = a.V + (int64_t)i * a.vstride + tc.j0;
            double acc[T];
#pragma unroll
            for (int c = 0; c < T; ++c) acc[c] = 0.0;
#pragma unroll
            for (int k = 0; k < PL; ++k) {
                if (rows.live(k)) {
                    double v[T];
                    tile_ld<T, F>(vb + rows.row(k) * a.ldv, tc.mask, v);
#pragma unroll
                    for (int c = 0; c < T; ++c) acc[c] = acc[c] + v[c] * wv[k][c];
                }
            }
#pragma unroll
            for (int c = 0; c < T; ++c) {
                const double sum = wave_fold(acc[c]);
                if ((threadIdx.x & 63) == 0) ws[i][c][threadIdx.x >> 6] = sum;
            }
        }
    };
    if (WIDE && tc.mask == FULL_MASK) body(std::true_type{});
    else body(std::false_type{});
    __syncthreads();
    // the running columns share the count (a resting one has none): block i of every column of the mask
    for (int q = threadIdx.x; q < tc.nmax * T; q += KRYLOV_LANES) {
        const int i = q / T, c = q % T;
        if (tc.mask >> c & 1u) a.part[((int64_t)i * a.s + tc.j0 + c) * a.cells + tc.cell] = (ws[i][c][0] + ws[i][c][1]) + (ws[i][c][2] + ws[i][c][3]);
    }
}

// ---- the projection: w <- w - coef_0 v_0 - coef_1 v_1 - ..., each product rounded and each difference rounded ---------
template <bool WIDE> __global__ __launch_bounds__(KRYLOV_LANES) void gmres_multi_project_kernel(const MColArgs a)
{
    const TileCols tc(a);
    if (tc.mask == 0) return;
    const Rows rows(tc.cell, a.n);
    double acc[T];
#pragma unroll
    for (int c = 0; c < T; ++c) acc[c] = 0.0;
    auto body = [&](auto fast) {
        constexpr bool F = decltype(fast)::value;
        double t[PL][T];
        load_rows<F>(rows, a.w + tc.j0, a.ldw, tc.mask, t);
        for (int i = 0; i < tc.nmax; ++i) {
            const double *vb = a.V + (int64_t)i * a.vstride + tc.j0;
            double h[T];
#pragma unroll
            for (int c = 0; c < T; ++c) h[c] = i < tc.nk[c] ? a.coef[(int64_t)(tc.j0 + c) * a.ldc + i] : 0.0; // uniform
#pragma unroll
            for (int k = 0; k < PL; ++k) {
                if (rows.live(k)) {
                    double v[T];
                    tile_ld<T, F>(vb + rows.row(k) * a.ldv, tc.mask, v);
#pragma unroll
                    for (int c = 0; c < T; ++c)
                        if (i < tc.nk[c]) t[k][c] = t[k][c] - h[c] * v[c];
                }
            }
        }
        store_rows<F>(rows, a.w + tc.j0, a.ldw, tc.mask, t);
        if (a.part) { // stage 1 of (w, w) over what was just written
#pragma unroll
            for (int k = 0; k < PL; ++k)
                if (rows.live(k)) {
#pragma unroll
                    for (int c = 0; c < T; ++c) acc[c] = acc[c] + t[k][c] * t[k][c];
                }
        }
    };
    if (WIDE && tc.mask == FULL_MASK) body(std::true_type{});
    else body(std::false_type{});
    if (a.part) tile_store<1>(acc, a.part, a.s, a.cells, tc.cell, tc.j0, tc.mask);
}

// ---- the combination: u = y_0 v_0, then u = u + y_l v_l ascending, rounded product and rounded sum ----------------------
template <bool WIDE> __global__ __launch_bounds__(KRYLOV_LANES) void gmres_multi_combine_kernel(const MColArgs a)
{
    const TileCols tc(a);
    if (tc.mask == 0) return;
    const Rows rows(tc.cell, a.n);
    auto body = [&](auto fast) {
        constexpr bool F = decltype(fast)::value;
        double t[PL][T];
#pragma unroll
        for (int k = 0; k < PL; ++k)
#pragma unroll
            for (int c = 0; c < T; ++c) t[k][c] = 0.0;
        for (int i = 0; i < tc.nmax; ++i) {
            const double *vb = a.V + (int64_t)i * a.vstride + tc.j0;
            double y[T];
#pragma unroll
            for (int c = 0; c < T; ++c) y[c] = i < tc.nk[c] ? a.coef[(int64_t)(tc.j0 + c) * a.ldc + i] : 0.0; // uniform
#pragma unroll
            for (int k = 0; k < PL; ++k) {
                if (rows.live(k)) {
                    double v[T];
                    tile_ld<T, F>(vb + rows.row(k) * a.ldv, tc.mask, v);
#pragma unroll
                    for (int c = 0; c < T; ++c)
                        if (i < tc.nk[c]) t[k][c] = i == 0 ? y[c] * v[c] : t[k][c] + y[c] * v[c];
                }
            }
        }
        store_rows<F>(rows, a.w + tc.j0, a.ldw, tc.mask, t);
    };
    if (WIDE && tc.mask == FULL_MASK) body(std::true_type{});
    else body(std::false_type{});
}

// ---- the plan's elementwise passes -------------------------------------------------------------------------------------
struct MVecArgs {
    int64_t n, cells, vstride, ldb, ldx;
    int s;
    double *blk, *part;
    double *V, *w, *z, *x; // V, w, z and u have leading dimension s; x has ldx, b has ldb
    const double *b, *dinv, *u;
};

struct TileAt {
    int64_t cell;
    int j0, w;
    __device__ __forceinline__ TileAt(int64_t cells, int s)
    {
        const TileId id = tile_id(cells, tiles(s));
        cell = id.block, j0 = (int)id.tile * T, w = s - j0 < T ? s - j0 : T;
    }
};

__device__ __forceinline__ const long long *iblock(const double *blk, int c) { return reinterpret_cast<const long long *>(blk) + (size_t)c * GMRES_BLOCK_SLOTS; }

// R = B - W (W = A X on entry), one rounded difference, left in W; stage 1 of (r, r) per column.  START: every column,
// and b_c == 0 writes x_c = 0 and r_c = 0 instead.  Otherwise: the columns a restart is due for.
template <bool START, bool WIDE> __global__ __launch_bounds__(KRYLOV_LANES) void gmres_multi_residual_kernel(const MVecArgs a)
{
    const TileAt at(a.cells, a.s);
    unsigned mask = 0, zmask = 0;
#pragma unroll
    for (int c = 0; c < T; ++c) {
        if (c < at.w) {
            const long long *ib = iblock(a.blk, at.j0 + c);
            if (START || (ib[GS_STATUS] == GMRES_RUNNING && ib[GS_COLS] == ib[GS_M] && ib[GS_PENDING] == 0)) mask |= 1u << c;
            if (START && ib[GS_ZERO_X] != 0) zmask |= 1u << c;
        }
    }
    if (mask == 0) return;
    double acc[T];
#pragma unroll
    for (int c = 0; c < T; ++c) acc[c] = 0.0;
    auto body = [&](auto fast) {
        constexpr bool F = decltype(fast)::value;
        row_walk(at.cell, a.n, [&](int64_t i) {
            double b[T], q[T], r[T];
            tile_ld<T, F>(a.b + i * a.ldb + at.j0, mask, b), tile_ld<T, F>(a.w + i * a.s + at.j0, mask, q);
            double *x = a.x + i * a.ldx + at.j0;
#pragma unroll
            for (int c = 0; c < T; ++c) {
                const bool zero = zmask >> c & 1u;
                if (zero) x[c] = 0.0;
                r[c] = zero ? 0.0 : b[c] - q[c];
                acc[c] = acc[c] + r[c] * r[c];
            }
            tile_st<T, F>(a.w + i * a.s + at.j0, mask, r);
        });
    };
    if (WIDE && mask == FULL_MASK) body(std::true_type{});
    else body(std::false_type{});
    tile_store<1>(acc, a.part, a.s, a.cells, at.cell, at.j0, mask);
}

// V_k[:, c] = W[:, c] / eta_c with k and eta from column c's block, and the next step's operand Z = V_k (JAC: dinv o V_k)
template <bool JAC, bool WIDE> __global__ __launch_bounds__(KRYLOV_LANES) void gmres_multi_normal_kernel(const MVecArgs a)
{
    const TileAt at(a.cells, a.s);
    unsigned mask = 0;
    double eta[T];
    int64_t off[T]; // where column c's block of V begins
    bool same = true;
    int64_t first_off = -1;
#pragma unroll
    for (int c = 0; c < T; ++c) {
        eta[c] = 1.0, off[c] = 0;
        if (c < at.w) {
            const long long *ib = iblock(a.blk, at.j0 + c);
            if (ib[GS_ACTIVE]) {
                mask |= 1u << c;
                eta[c] = a.blk[(size_t)(at.j0 + c) * GMRES_BLOCK_SLOTS + GS_ETA];
                off[c] = ib[GS_COLS] * a.vstride;
                if (first_off < 0) first_off = off[c];
                same = same && off[c] == first_off;
            }
        }
    }
    if (mask == 0) return;
    if (WIDE && mask == FULL_MASK && same) { // the running columns share the count: one block of V for the whole tile
        double *vk = a.V + first_off;
        row_walk(at.cell, a.n, [&](int64_t i) {
            double v[T];
            tile_ld<T, true>(a.w + i * a.s + at.j0, mask, v);
#pragma unroll
            for (int c = 0; c < T; ++c) v[c] = v[c] / eta[c];
            tile_st<T, true>(vk + i * a.s + at.j0, mask, v);
            if (JAC) {
                const double di = a.dinv[i];
#pragma unroll
                for (int c = 0; c < T; ++c) v[c] = di * v[c];
            }
            tile_st<T, true>(a.z + i * a.s + at.j0, mask, v);
        });
    } else {
        row_walk(at.cell, a.n, [&](int64_t i) {
            double v[T];
            tile_ld<T, false>(a.w + i * a.s + at.j0, mask, v);
            double *vrow = a.V + i * a.s + at.j0;
#pragma unroll
            for (int c = 0; c < T; ++c) {
                v[c] = v[c] / eta[c];
                if (mask >> c & 1u) vrow[off[c] + c] = v[c];
            }
            if (JAC) {
                const double di = a.dinv[i];
#pragma unroll
                for (int c = 0; c < T; ++c) v[c] = di * v[c];
            }
            tile_st<T, false>(a.z + i * a.s + at.j0, mask, v);
        });
    }
}

// X = X + Z with Z = U (JAC: the rounded dinv o U), on the columns this close acts for
template <bool JAC, bool WIDE> __global__ __launch_bounds__(KRYLOV_LANES) void gmres_multi_x_kernel(const MVecArgs a)
{
    const TileAt at(a.cells, a.s);
    unsigned mask = 0;
#pragma unroll
    for (int c = 0; c < T; ++c)
        if (c < at.w && iblock(a.blk, at.j0 + c)[GS_CLOSE]) mask |= 1u << c;
    if (mask == 0) return;
    auto body = [&](auto fast) {
        constexpr bool F = decltype(fast)::value;
        row_walk(at.cell, a.n, [&](int64_t i) {
            double x[T], u[T];
            tile_ld<T, F>(a.x + i * a.ldx + at.j0, mask, x), tile_ld<T, F>(a.u + i * a.s + at.j0, mask, u);
            if (JAC) {
                const double di = a.dinv[i];
#pragma unroll
                for (int c = 0; c < T; ++c) u[c] = di * u[c];
            }
#pragma unroll
            for (int c = 0; c < T; ++c) x[c] = x[c] + u[c];
            tile_st<T, F>(a.x + i * a.ldx + at.j0, mask, x);
        });
    };
    if (WIDE && mask == FULL_MASK) body(std::true_type{});
    else body(std::false_type{});
}

// the first kernel of a close, one lane a column (gmres_fold.h's text)
__global__ void gmres_multi_close_kernel(int s, double *blk, double *mat)
{
    const int c = (int)threadIdx.x;
    if (c < s) gmres_close_lane(blk + (size_t)c * GMRES_BLOCK_SLOTS, mat + (size_t)c * GMRES_MULTI_MATRIX_STRIDE);
}

// ---- stage 2, which is also the scalar step: one workgroup a column (gmres_fold.h's text) ---------------------------------
__global__ __launch_bounds__(KRYLOV_LANES) void gmres_multi_fold_kernel(int op, int nd, int s, int64_t cells, const double *part, double *blk,
                                                                       double *mat, double *out, double rtol, double atol, long long max_iter, int m)
{
    __shared__ double ws[GMRES_MAX_DOTS][4];
    const int c = (int)blockIdx.x;
    if (blk) blk += (size_t)c * GMRES_BLOCK_SLOTS, mat += (size_t)c * GMRES_MULTI_MATRIX_STRIDE;
    long long *ib = reinterpret_cast<long long *>(blk);
    if (op == GF_OUT) {
        if (blk && ib[GS_STATUS] != GMRES_RUNNING) return; // the stand-alone dots of a column that rests
    } else if (!gmres_fold_acts(op, ib)) {
        return;
    }
    if (op == GF_H1 || op == GF_H2) nd = (int)ib[GS_COLS] + 1;
    gmres_fold_sums(nd, cells, part + (int64_t)c * cells, (int64_t)s * cells, ws); // dot q of column c at part[(q * s + c) * cells]
    __syncthreads();
    if (threadIdx.x != 0) return;
    gmres_fold_lane0(op, nd, ws, blk, mat, out ? out + c : nullptr, s, rtol, atol, max_iter, m);
}

// ---- launches ----------------------------------------------------------------------------------------------------------
struct GmresMultiPlan : MultiPlanBase {
    int m = 0;
    int64_t vstride = 0;
    size_t matrix_bytes = 0;
    double *mat = nullptr; // scalar blocks | small matrices | partials | the SpMM's workspace | V_0 .. V_m, W, U, Z [, T]
    int pos = 0; // steps enqueued since the chain's last restart (or start): where the next close and restart belong
    const double *b = nullptr;
    int64_t ldb = 0;
    double *block(int k) const { return vec + (size_t)k * (size_t)vstride; }
    double *w() const { return block(m + 1); }
    double *u() const { return block(m + 2); }
    double *z() const { return block(m + 3); }
    double *t() const { return block(m + 4); } // the close's second block, of a kind that cannot run in place
    bool second() const { return pre.applied() && !pre.in_place(); }
};

inline unsigned grid_of(int64_t cells, int s) { return (unsigned)tile_grid(cells, s); }

void launch_dots(hipStream_t st, const MColArgs &a)
{
    if (wide16(a.V, a.ldv) && ((a.vstride * 8) & 15) == 0 && wide16(a.w, a.ldw)) gmres_multi_dots_kernel<true><<<grid_of(a.cells, a.s), KRYLOV_LANES, 0, st>>>(a);
    else gmres_multi_dots_kernel<false><<<grid_of(a.cells, a.s), KRYLOV_LANES, 0, st>>>(a);
}

void launch_project(hipStream_t st, const MColArgs &a)
{
    if (wide16(a.V, a.ldv) && ((a.vstride * 8) & 15) == 0 && wide16(a.w, a.ldw)) gmres_multi_project_kernel<true><<<grid_of(a.cells, a.s), KRYLOV_LANES, 0, st>>>(a);
    else gmres_multi_project_kernel<false><<<grid_of(a.cells, a.s), KRYLOV_LANES, 0, st>>>(a);
}

void launch_combine(hipStream_t st, const MColArgs &a)
{
    if (wide16(a.V, a.ldv) && ((a.vstride * 8) & 15) == 0 && wide16(a.w, a.ldw)) gmres_multi_combine_kernel<true><<<grid_of(a.cells, a.s), KRYLOV_LANES, 0, st>>>(a);
    else gmres_multi_combine_kernel<false><<<grid_of(a.cells, a.s), KRYLOV_LANES, 0, st>>>(a);
}

void launch_fold(hipStream_t st, int op, int nd, int s, int64_t cells, const double *part, double *blk, double *mat, double *out, double rtol = 0.0,
                 double atol = 0.0, int64_t max_iter = 0, int m = 0)
{
    gmres_multi_fold_kernel<<<(unsigned)s, KRYLOV_LANES, 0, st>>>(op, nd, s, cells, part, blk, mat, out, rtol, atol, (long long)max_iter, m);
}

void fold(const GmresMultiPlan *p, hipStream_t st, int op, double rtol = 0.0, double atol = 0.0, int64_t max_iter = 0)
{
    launch_fold(st, op, 1, p->s, p->cells, p->part, p->blk, p->mat, nullptr, rtol, atol, max_iter, p->m);
}

MColArgs col_args(const GmresMultiPlan *p, int mode, const double *coef, double *w, double *part)
{
    return MColArgs{p->n, p->cells, p->s, p->vstride, p->s, GMRES_MULTI_MATRIX_STRIDE, p->s, 0, mode, p->vec, coef, w, part, p->blk};
}

MVecArgs vec_args(const GmresMultiPlan *p)
{
    return MVecArgs{p->n, p->cells, p->vstride, p->ldb, p->ldx, p->s, p->blk, p->part, p->vec, p->w(), p->z(), p->x, p->b, p->pre.values, p->u()};
}

// the plan's own blocks have leading dimension s and 256-byte aligned bases: wide when s is even
bool plan_wide(const GmresMultiPlan *p) { return wide16(p->vec, p->s) && ((p->vstride * 8) & 15) == 0; }

void normalise(const GmresMultiPlan *p, hipStream_t st)
{
    const unsigned grid = grid_of(p->cells, p->s);
    const bool wide = plan_wide(p);
    const MVecArgs a = vec_args(p);
    if (p->pre.jacobi()) {
        if (wide) gmres_multi_normal_kernel<true, true><<<grid, KRYLOV_LANES, 0, st>>>(a);
        else gmres_multi_normal_kernel<true, false><<<grid, KRYLOV_LANES, 0, st>>>(a);
    } else {
        if (wide) gmres_multi_normal_kernel<false, true><<<grid, KRYLOV_LANES, 0, st>>>(a);
        else gmres_multi_normal_kernel<false, false><<<grid, KRYLOV_LANES, 0, st>>>(a);
    }
}

template <bool START> void residual(const GmresMultiPlan *p, hipStream_t st)
{
    const unsigned grid = grid_of(p->cells, p->s);
    const bool wide = plan_wide(p) && wide16(p->b, p->ldb); // x is written double by double
    const MVecArgs a = vec_args(p);
    if (wide) gmres_multi_residual_kernel<START, true><<<grid, KRYLOV_LANES, 0, st>>>(a);
    else gmres_multi_residual_kernel<START, false><<<grid, KRYLOV_LANES, 0, st>>>(a);
}

int step_launches(const GmresMultiPlan *p, hipStream_t st)
{
    const bool app = p->pre.applied();
    int rc;
    // an applied M^-1 runs on ALL columns, into U, which is free between two closes
    if (app && (rc = p->pre.apply_multi(st, p->s, p->z(), p->s, p->u(), p->s)) != SBLAS_OK) return rc;
    if ((rc = product(p, st, app ? p->u() : p->z(), p->s, p->w())) != SBLAS_OK) return rc;
    launch_dots(st, col_args(p, MODE_FIRST, nullptr, p->w(), p->part));
    fold(p, st, GF_H1);
    launch_project(st, col_args(p, MODE_ACTIVE, p->mat + GM_H, p->w(), nullptr));
    launch_dots(st, col_args(p, MODE_ACTIVE, nullptr, p->w(), p->part));
    fold(p, st, GF_H2);
    launch_project(st, col_args(p, MODE_ACTIVE, p->mat + GM_H2, p->w(), p->part));
    fold(p, st, GF_STEP);
    normalise(p, st);
    return SBLAS_OK;
}

int close_launches(const GmresMultiPlan *p, hipStream_t st)
{
    const unsigned grid = grid_of(p->cells, p->s);
    gmres_multi_close_kernel<<<1, 64, 0, st>>>(p->s, p->blk, p->mat);
    launch_combine(st, col_args(p, MODE_CLOSE, p->mat + GM_Y, p->u(), nullptr));
    MVecArgs a = vec_args(p);
    if (p->pre.applied()) { // in place where M^-1 may run so; else the correction is read from the second block
        double *out = p->pre.in_place() ? p->u() : p->t();
        const int rc = p->pre.apply_multi(st, p->s, p->u(), p->s, out, p->s);
        if (rc != SBLAS_OK) return rc;
        a.u = out;
    }
    const bool wide = plan_wide(p) && wide16(p->x, p->ldx);
    if (p->pre.jacobi()) {
        if (wide) gmres_multi_x_kernel<true, true><<<grid, KRYLOV_LANES, 0, st>>>(a);
        else gmres_multi_x_kernel<true, false><<<grid, KRYLOV_LANES, 0, st>>>(a);
    } else {
        if (wide) gmres_multi_x_kernel<false, true><<<grid, KRYLOV_LANES, 0, st>>>(a);
        else gmres_multi_x_kernel<false, false><<<grid, KRYLOV_LANES, 0, st>>>(a);
    }
    return SBLAS_OK;
}

int restart_launches(const GmresMultiPlan *p, hipStream_t st)
{
    const int rc = product(p, st, p->x, p->ldx, p->w());
    if (rc != SBLAS_OK) return rc;
    residual<false>(p, st);
    fold(p, st, GF_BEGIN_RESTART);
    normalise(p, st);
    return SBLAS_OK;
}

// what the stand-alone entry points refuse: k basis blocks at V, an n x s block at w, column-wise coefficients at coef
bool blocks_ok(int64_t n, int nrhs, int k, const double *V, int64_t ldv, int64_t stride, const void *w, int64_t ldw, const void *scalars)
{
    if (n < 0 || n > INT_MAX || !gmres_multi_width_ok(nrhs) || k < 1 || k > GMRES_MAX_DOTS) return false;
    if (ldv < nrhs || ldw < nrhs) return false;
    if (k > 1 && (stride < 0 || (n > 0 && stride / ldv < n))) return false; // a block stride below n * ldv
    if (n > 0 && (!V || !w)) return false;
    return ((reinterpret_cast<uintptr_t>(V) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(scalars)) & 7u) == 0;
}

void launch_counts(const GmresMultiPlan *p, int64_t out[4], int64_t *cycle)
{
    int64_t lower[12], upper[12], mi[4] = {0, 0, 0, 0};
    p->pre.info(lower, upper);
    int64_t first = 0, second = 0;
    if (precond_multi_pair(p->pre.kind)) first = lower[5], second = upper[5];
    else if (precond_multi_applied(p->pre.kind) && sblas_hip_amg_plan_multi_info(p->pre.lower, mi) == SBLAS_OK) first = mi[2];
    *cycle = sblas_gmres_multi_launches(p->m, p->pre.kind, 0, first, second, out);
}

} // namespace

extern "C" {

size_t sblas_hip_gmres_multi_dots_workspace(int64_t n, int nrhs, int k)
{
    if (n < 0 || !gmres_multi_width_ok(nrhs) || k < 1 || k > GMRES_MAX_DOTS) return 0;
    const size_t sums = (size_t)k * (size_t)nrhs * (size_t)krylov_cells(n);
    return (sums ? sums : 1) * sizeof(double); // never 0: a workspace is always asked for
}

int sblas_hip_gmres_multi_dots_f64(int dev, void *stream, int64_t n, int nrhs, int k, const double *V, int64_t ldv, int64_t block_stride,
                                   const double *W, int64_t ldw, const double *scalars, double *out, void *workspace, size_t workspace_bytes)
{
    if (!blocks_ok(n, nrhs, k, V, ldv, block_stride, W, ldw, scalars) || !out) return SBLAS_E_INVALID;
    if (!workspace || workspace_bytes < sblas_hip_gmres_multi_dots_workspace(n, nrhs, k)) return SBLAS_E_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(out)) & 7u) return SBLAS_E_INVALID;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    hipStream_t st = (hipStream_t)stream;
    const int64_t cells = krylov_cells(n);
    double *part = static_cast<double *>(workspace);
    if (cells > 0) launch_dots(st, MColArgs{n, cells, ldv, block_stride, ldw, 0, nrhs, k, MODE_FREE, V, nullptr, const_cast<double *>(W), part, scalars});
    launch_fold(st, GF_OUT, k, nrhs, cells, part, const_cast<double *>(scalars), nullptr, out);
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_gmres_multi_project_f64(int dev, void *stream, int64_t n, int nrhs, int k, const double *V, int64_t ldv, int64_t block_stride,
                                      const double *H, int64_t ldh, double *W, int64_t ldw, const double *scalars, double *partial)
{
    if (!blocks_ok(n, nrhs, k, V, ldv, block_stride, W, ldw, scalars) || !H || ldh < k) return SBLAS_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(H) | reinterpret_cast<uintptr_t>(partial)) & 7u) return SBLAS_E_INVALID;
    if (n == 0) return SBLAS_OK;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    launch_project((hipStream_t)stream, MColArgs{n, krylov_cells(n), ldv, block_stride, ldw, ldh, nrhs, k, MODE_FREE, V, H, W, partial, scalars});
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_gmres_multi_combine_f64(int dev, void *stream, int64_t n, int nrhs, int k, const double *V, int64_t ldv, int64_t block_stride,
                                      const double *Y, int64_t ldy, double *U, int64_t ldu, const double *scalars)
{
    if (!blocks_ok(n, nrhs, k, V, ldv, block_stride, U, ldu, scalars) || !Y || ldy < k) return SBLAS_E_INVALID;
    if (reinterpret_cast<uintptr_t>(Y) & 7u) return SBLAS_E_INVALID;
    if (n == 0) return SBLAS_OK;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    launch_combine((hipStream_t)stream, MColArgs{n, krylov_cells(n), ldv, block_stride, ldu, ldy, nrhs, k, MODE_FREE, V, Y, U, nullptr, scalars});
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_gmres_multi_plan_create(int dev, void *stream, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx, int nrhs,
                                      int restart, int precond, const void *lower_plan, const void *upper_plan, void **plan_out)
{
    if (!plan_out) return SBLAS_E_INVALID;
    *plan_out = nullptr;
    if (!gmres_multi_width_ok(nrhs) || !gmres_multi_restart_ok(restart)) return SBLAS_E_INVALID;
    // precond_rule.h: a kind that rides in the kernels takes no plan, AMG its own, ILU(0) its pair; every other kind is refused
    if (precond_multi(precond) ? (lower_plan || upper_plan)
        : precond_multi_applied(precond) ? (!lower_plan || upper_plan)
        : precond_multi_pair(precond) ? (!lower_plan || !upper_plan) : true)
        return SBLAS_E_INVALID;
    std::unique_ptr<GmresMultiPlan> p(new GmresMultiPlan);
    p->m = restart;
    int rc = multi_bind(p.get(), dev, stream, n, nnz, rowptr, colidx, nrhs, precond, lower_plan, upper_plan);
    if (rc != SBLAS_OK) return rc;
    p->n_blocks = restart + 1 + GMRES_MULTI_FIXED_BLOCKS + (p->second() ? 1 : 0);
    rc = multi_layout(p.get(), stream, {{&p->blk, &p->scalar_bytes, (size_t)nrhs * GMRES_BLOCK_SLOTS * 8, 1},
                                        {&p->mat, &p->matrix_bytes, (size_t)nrhs * (size_t)GMRES_MULTI_MATRIX_STRIDE * 8, 1},
                                        {&p->part, &p->partial_bytes, (size_t)(restart + 1) * (size_t)nrhs * (size_t)p->cells * 8, 1},
                                        multi_workspace(p.get()),
                                        {&p->vec, &p->block_bytes, (size_t)n * (size_t)nrhs * 8, p->n_blocks}});
    if (rc != SBLAS_OK) return rc;
    p->vstride = (int64_t)(p->block_bytes / 8);
    *plan_out = p.release();
    return SBLAS_OK;
}

int sblas_hip_gmres_multi_plan_info(const void *plan, int64_t out[16])
{
    if (!plan || !out) return SBLAS_E_INVALID;
    const GmresMultiPlan *p = static_cast<const GmresMultiPlan *>(plan);
    int64_t launches[4] = {0, 0, 0, 0}, cycle = 0;
    launch_counts(p, launches, &cycle);
    out[0] = p->n, out[1] = p->nnz, out[2] = p->m, out[3] = p->pre.kind, out[4] = p->s, out[5] = p->n_blocks;
    out[6] = (int64_t)p->block_bytes, out[7] = (int64_t)p->partial_bytes, out[8] = (int64_t)p->scalar_bytes, out[9] = (int64_t)p->matrix_bytes;
    out[10] = (int64_t)p->ws_bytes, out[11] = (int64_t)p->bytes;
    out[12] = launches[0], out[13] = launches[1], out[14] = launches[2], out[15] = cycle;
    return SBLAS_OK;
}

int sblas_hip_gmres_multi_plan_block(const void *plan, void *stream, int k, double *out)
{
    const GmresMultiPlan *p = static_cast<const GmresMultiPlan *>(plan);
    if (!p || k < 0 || k >= p->n_blocks) return SBLAS_E_INVALID;
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
    if (p->n == 0) return SBLAS_OK;
    if (!out) return SBLAS_E_INVALID;
    const size_t bytes = (size_t)p->n * (size_t)p->s * 8;
    return hipMemcpyAsync(out, p->block(k), bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream) == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_gmres_multi_plan_destroy(void *plan)
{
    delete static_cast<GmresMultiPlan *>(plan);
    return SBLAS_OK;
}

int sblas_hip_gmres_multi_start(void *plan, void *stream, const double *val, const double *lu_or_dinv, const double *B, int64_t ldb, double *X,
                                int64_t ldx, double rtol, double atol, int64_t max_iter)
{
    GmresMultiPlan *p = static_cast<GmresMultiPlan *>(plan);
    const MultiStart go = multi_start(p, val, lu_or_dinv, B, ldb, X, ldx, rtol, atol, max_iter);
    if (go != MULTI_GO) return go == MULTI_EMPTY ? SBLAS_OK : SBLAS_E_INVALID;
    p->b = B, p->ldb = ldb, p->pos = 0;
    hipStream_t st = (hipStream_t)stream;
    // The work blocks start every solve from zero.  A column that is frozen from the start is never written, yet the SpMM
    // multiplies it -- and a non-finite value a previous solve left there would select other SpMM kernels for the whole
    // product.  So the bits of a solve are a function of its own operands alone.
    if (hipMemsetAsync(p->w(), 0, (size_t)(p->n_blocks - p->m - 1) * p->block_bytes, st) != hipSuccess) return SBLAS_E_HIP;
    // (b_c, b_c) by the multi-dot of one block: the single dot's bits on every column
    launch_dots(st, MColArgs{p->n, p->cells, ldb, 0, ldb, 0, p->s, 1, MODE_FREE, B, nullptr, const_cast<double *>(B), p->part, nullptr});
    fold(p, st, GF_START_B, rtol, atol, max_iter);
    const int rc = product(p, st, X, ldx, p->w());
    if (rc != SBLAS_OK) return rc;
    residual<true>(p, st);
    fold(p, st, GF_BEGIN_START);
    normalise(p, st);
    if (hipGetLastError() != hipSuccess) return SBLAS_E_HIP;
    p->started = true;
    return SBLAS_OK;
}

int sblas_hip_gmres_multi_iterate(void *plan, void *stream, int64_t k)
{
    GmresMultiPlan *p = static_cast<GmresMultiPlan *>(plan);
    if (!p || k < 0 || !p->started) return SBLAS_E_INVALID;
    if (p->dev != resolve_device(-1)) return SBLAS_E_INVALID;
    if (p->n == 0) return SBLAS_OK;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    for (int64_t it = 0; it < k; ++it) {
        if ((rc = step_launches(p, st)) != SBLAS_OK) return rc;
        if (++p->pos == p->m) { // the cycle is full (or the columns are frozen and ignore all this)
            p->pos = 0;
            if ((rc = close_launches(p, st)) != SBLAS_OK || (rc = restart_launches(p, st)) != SBLAS_OK) return rc;
        }
    }
    if ((rc = close_launches(p, st)) != SBLAS_OK) return rc; // acts only for the columns that ended inside this batch
    return hipGetLastError() == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_gmres_multi_status(const void *plan, void *stream, double *out)
{
    static const StatusSlot table[8] = {{GS_STATUS, true}, {GS_ITER, true}, {GS_RNORM, false}, {GS_BNORM, false},
                                        {GS_RESTARTS, true}, {GS_COLS, true}, {GS_ETA, false}, {GS_WHICH, true}};
    return multi_status<GMRES_BLOCK_SLOTS>(static_cast<const GmresMultiPlan *>(plan), stream, out, table);
}

} // extern "C"
