// attention.hip -- fused attention on a CSR pattern for gfx950 (wave64): O = softmax(scale * Q K^T on A's pattern) V in
// one pass over each row, its backward, and their C-ABI entry points (include/sblas_hip.h, "Fused attention").
// DESIGN.md 3.17.
//
//   forward    s[e] = <Q[i, :], K[c(e), :]>,  t = scale * s,  m = max t,  z = sum exp(t - m),  p = exp(t - m) / z,
//              O[i, :] = sum_e p[e] V[c(e), :]                                     row_max[i] = m, row_sum[i] = z
//   backward   t, p again from Q, K, m, z;  dp[e] = <dO[i, :], V[c(e), :]>,  D = sum p dp,  dS = (scale * p) * (dp - D),
//              dQ[i, :] = sum_e dS[e] K[c(e), :];  P and dS written out on request
//
//   attn_rows_kernel<BWD>          a wave per AT_ROWS consecutive rows; every row of at most ROW_SUPER = 4096 entries
//   attn_long_kernel<BWD, PHASE>   a wave per ROW_SUPER consecutive entry positions; the rows longer than ROW_SUPER
//
// A workgroup is ONE wave: __syncthreads() orders the wave's own LDS traffic and waits for nobody.  Nothing nnz-sized is
// written unless the caller asks the backward for P / dS.  Only rowptr is read to find the work, never a host copy.
//
// A run is a row of at most 4096 entries, or one supercell (4096 entries counted from the ROW's start, the last one
// shorter) of a longer row; a wave takes a run in segments of AT_SEG = 512 entries (8 cells).  Per segment: the column
// indices go to LDS; lane groups of G = sddmm_group(d) lanes form the dot products exactly as sddmm_kernel does for
// k = d (pieces q = l, l + G, ..., one fma per element into +0, the group butterfly) and leave scale * s in LDS; then lane
// j % 64 owns entry j, as in softmax.hip.  A run of one segment computes its scores once and keeps them in LDS; a longer
// run evaluates them again for each of its passes (max, sum, output), which costs the arithmetic twice more and no
// memory.  Rows longer than 4096: the workgroup whose block of positions holds a supercell's first entry owns it, and
// the per-supercell max / sum / dot and partial output rows go to the workspace (softmax.hip's slot rule), one launch a
// phase: max, sum, output, fold.
//
// Orders (functions of the row's length L, d and dv alone; the bits follow the row, not its place):
//   - dot products: DESIGN 3.15 for k = d (scores) and k = dv (dp), alpha = 1, beta = 0.
//   - max, z, D: DESIGN 3.16's cell / supercell tree over the row's entries numbered from its start; supercell figures
//     added left to right into +0.  t = scale * s, t - m, e / z, fma(p, dp, +0), (scale * p) * (dp - D): one rounding each.
//   - O[i, c] (dQ[i, c] alike, with dS and K): W = the power of two in [4, 64] that is >= min(dv, 64), NG = 64 / W.
//     Inside a run, entry j (counted from the run's start) belongs to group j % NG; a group's accumulator starts at +0
//     and takes acc = fma(p[j], V[c(j), c], acc) for its entries in ascending j.  The NG accumulators are then folded by the
//     butterfly acc += acc[g ^ 1], acc += acc[g ^ 2], ... over the groups.  That is the run's row; a row of several runs
//     is +0 plus its runs' rows, left to right.  (An accumulator is never -0, so the +0 changes nothing.)
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include "../../include/sblas_hip.h"
#include "capi_util.h"
#include "kernels.h"
#include "rowwise.h"

#pragma clang fp contract(off)

namespace sblas {
namespace {

constexpr int AT_THREADS = 64; // one wave a workgroup
constexpr int AT_SEG = 512;    // entries a wave scores at a time: 8 cells
constexpr int AT_CELLS = AT_SEG / ROW_CELL;
constexpr int AT_ROWS = 4;     // consecutive rows of a wave in the rows kernel
constexpr int AT_MAXW = SDDMM_SLICE; // widest Q / K / V row of the fused entry points: one SDDMM slice

// lanes per entry of the accumulation, as a shift: the power of two in [4, 64] that covers min(n, 64) columns
int width_shift(int64_t n) { return n <= 4 ? 2 : n <= 8 ? 3 : n <= 16 ? 4 : n <= 32 ? 5 : 6; }

struct Args {
    int rows, nnz;
    const int *rowptr, *colidx;
    const double *Q, *K, *V, *dO;
    int64_t ldq, ldk, ldv, lddo;
    int d, dv;
    int gd, gv;         // sddmm_group_shift(d), sddmm_group_shift(dv)
    int wshift, wn;     // the accumulation: width_shift and the columns of the output row (forward dv, backward d)
    int vec_qk, vec_ov; // 16-byte loads for the score / dp dot products
    double scale;
    double *O;          // forward O, backward dQ (may be null there)
    int64_t ldo;
    double *row_max, *row_sum; // forward: written when not null; backward: read
    double *P, *dS;     // backward, on request
    double *pmax, *psum, *part; // workspace: per-supercell max, sum (backward: dot), partial output rows of `wpart` doubles
    int wpart;
};

template <bool BWD> struct Lds {
    double sc[AT_SEG];           // scores, then leaves, then probabilities (backward: dS)
    double dp[BWD ? AT_SEG : 1]; // backward only
    int cl[AT_SEG];
};

__device__ __forceinline__ double group_sum_rt(double s, int gshift)
{
    switch (gshift) {
    case 1: return group_sum<2>(s);
    case 2: return group_sum<4>(s);
    case 3: return group_sum<8>(s);
    case 4: return group_sum<16>(s);
    default: return s;
    }
}

// the pieces q = l, l + G, l + 2G, l + 3G of a row of k elements (sddmm_kernel's x[] / y[]; its PASSES only drops rounds
// that hold no element)
template <bool VEC> __device__ __forceinline__ void load_pieces(double2 (&x)[4], const double *__restrict__ row, int gshift, int l, int k)
{
#pragma unroll
    for (int p = 0; p < 4; ++p) x[p] = load_piece<VEC, false>(row, 2 * ((p << gshift) + l), k);
}
__device__ __forceinline__ void load_row(double2 (&x)[4], const double *__restrict__ row, int gshift, int lane, int k, int vec)
{
    const int l = lane & ((1 << gshift) - 1);
    if (vec) load_pieces<true>(x, row, gshift, l, k);
    else load_pieces<false>(x, row, gshift, l, k);
}

// out[j] = (SCALE ? scale * s : s), s = <x, Y[cl[j], :]> for the n entries of a segment; G = 1 << gshift lanes an entry
template <bool SCALE>
__device__ __forceinline__ void dot_segment(const double2 (&x)[4], const double *__restrict__ Y, int64_t ldy, int k, int gshift, int vec,
                                            const int *cl, int n, double scale, double *out, int lane)
{
    const int ng = 64 >> gshift, g = lane >> gshift, l = lane & ((1 << gshift) - 1);
    for (int jb = 0; jb < n; jb += ng) {
        const int j = jb + g;
        const bool on = j < n; // the same for all lanes of a group
        const double *yrow = Y + (int64_t)(on ? cl[j] : 0) * ldy;
        double2 y[4];
        if (vec) load_pieces<true>(y, yrow, gshift, l, on ? k : 0);
        else load_pieces<false>(y, yrow, gshift, l, on ? k : 0);
        double s = 0.0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            s = fma(x[p].x, y[p].x, s); // an element at or beyond k: both factors are the +0 load_piece left
            s = fma(x[p].y, y[p].y, s);
        }
        s = group_sum_rt(s, gshift);
        if (on && l == 0) out[j] = SCALE ? scale * s : s;
    }
}

// a0 (column c0) and a1 (column c0 + 64) of group g take the entries j = g, g + NG, ... of a segment, in that order
__device__ __forceinline__ void accumulate(const double *w, const int *cl, int n, const double *__restrict__ Y, int64_t ldy, int ncol,
                                           int wshift, int lane, double &a0, double &a1)
{
    const int c0 = lane & ((1 << wshift) - 1), g = lane >> wshift, ng = 64 >> wshift;
    const bool on0 = c0 < ncol, on1 = c0 + 64 < ncol;
#pragma unroll 4
    for (int j = g; j < n; j += ng) {
        const double p = w[j];
        const double *yrow = Y + (int64_t)cl[j] * ldy;
        if (on0) a0 = fma(p, yrow[c0], a0);
        if (on1) a1 = fma(p, yrow[c0 + 64], a1);
    }
}
__device__ __forceinline__ double fold_groups(double a, int wshift)
{
    for (int o = 1 << wshift; o < 64; o <<= 1) a += __shfl_xor(a, o, 64);
    return a;
}

enum { RUN_ROW = 0, RUN_MAX = 1, RUN_SUM = 2, RUN_OUT = 3 }; // backward: RUN_SUM is the dot D, there is no RUN_MAX

// The n <= AT_SEG entries from `base` on: column indices, scores and (backward, when wanted) dp into LDS
template <bool BWD>
__device__ __forceinline__ void load_segment(const Args &a, Lds<BWD> &s, int lane, const double2 (&q)[4], const double2 (&g)[4], int64_t base,
                                             int n, bool need_dp)
{
    __syncthreads(); // what the segment before left in LDS has been read
    for (int j = lane; j < n; j += 64) s.cl[j] = a.colidx[base + j];
    __syncthreads();
    dot_segment<true>(q, a.K, a.ldk, a.d, a.gd, a.vec_qk, s.cl, n, a.scale, s.sc, lane);
    if (BWD && need_dp) dot_segment<false>(g, a.V, a.ldv, a.dv, a.gv, a.vec_ov, s.cl, n, 1.0, s.dp, lane);
    __syncthreads();
}

// One run (cnt <= ROW_SUPER entries from e0 on) of row r, forward.  RUN_ROW: the whole row, m and z found here.
// RUN_MAX -> m.  RUN_SUM (m given) -> z, the run's sum.  RUN_OUT (m, z given) -> o0, o1.  o0 / o1: columns lane % W and
// lane % W + 64 of the run's output row, the same in every group.
template <int MODE>
__device__ __forceinline__ void forward_run(const Args &a, Lds<false> &s, int lane, int64_t r, int64_t e0, int cnt, double &m, double &z,
                                            double &o0, double &o1)
{
    double2 q[4];
    if (cnt > 0) load_row(q, a.Q + r * a.ldq, a.gd, lane, a.d, a.vec_qk);
    const int nseg = (cnt + AT_SEG - 1) / AT_SEG;
    const bool keep = MODE == RUN_ROW && nseg == 1; // the scores stay in LDS from pass to pass
    if (MODE == RUN_ROW || MODE == RUN_MAX) {
        m = NEG_INF;
        for (int sg = 0; sg < nseg; ++sg) {
            const int n = min(AT_SEG, cnt - sg * AT_SEG);
            load_segment<false>(a, s, lane, q, q, e0 + (int64_t)sg * AT_SEG, n, false);
#pragma unroll
            for (int c = 0; c < AT_CELLS; ++c) {
                const int i = c * ROW_CELL + lane;
                if (i < n) m = nmax(m, s.sc[i]);
            }
        }
        m = fold_max<64>(m);
        if (MODE == RUN_MAX) return;
    }
    if (MODE == RUN_ROW || MODE == RUN_SUM) {
        double cs = 0.0; // lane c holds the sum of cell c of the run
        for (int sg = 0; sg < nseg; ++sg) {
            const int n = min(AT_SEG, cnt - sg * AT_SEG);
            if (!keep) load_segment<false>(a, s, lane, q, q, e0 + (int64_t)sg * AT_SEG, n, false);
#pragma unroll
            for (int c = 0; c < AT_CELLS; ++c) {
                if (c * ROW_CELL < n) {
                    const int i = c * ROW_CELL + lane;
                    const double leaf = i < n ? exp(s.sc[i] - m) : 0.0;
                    if (keep && i < n) s.sc[i] = leaf;
                    const double sum = fold_sum<64>(leaf);
                    if (lane == sg * AT_CELLS + c) cs = sum;
                }
            }
        }
        z = fold_sum<64>(cs);
        if (MODE == RUN_SUM) return;
    }
    o0 = o1 = 0.0;
    for (int sg = 0; sg < nseg; ++sg) {
        const int n = min(AT_SEG, cnt - sg * AT_SEG);
        if (!keep) load_segment<false>(a, s, lane, q, q, e0 + (int64_t)sg * AT_SEG, n, false);
#pragma unroll
        for (int c = 0; c < AT_CELLS; ++c) {
            const int i = c * ROW_CELL + lane;
            if (i < n) s.sc[i] = keep ? s.sc[i] / z : fwd_out(s.sc[i], m, z);
        }
        __syncthreads();
        accumulate(s.sc, s.cl, n, a.V, a.ldv, a.dv, a.wshift, lane, o0, o1);
    }
    o0 = fold_groups(o0, a.wshift), o1 = fold_groups(o1, a.wshift);
}

// One run of row r, backward; m, z: the row's.  RUN_ROW: the whole row.  RUN_SUM -> D, the run's sum of p * dp.  RUN_OUT
// (D given): P / dS written, o0, o1 the run's dQ row.  Without dQ and dS no dp is formed and D is not needed.
template <int MODE>
__device__ __forceinline__ void backward_run(const Args &a, Lds<true> &s, int lane, int64_t r, int64_t e0, int cnt, double m, double z,
                                             double &D, double &o0, double &o1)
{
    const bool need_dp = a.O || a.dS;
    double2 q[4], g[4];
    if (cnt > 0) {
        load_row(q, a.Q + r * a.ldq, a.gd, lane, a.d, a.vec_qk);
        if (need_dp) load_row(g, a.dO + r * a.lddo, a.gv, lane, a.dv, a.vec_ov);
    }
    const int nseg = (cnt + AT_SEG - 1) / AT_SEG;
    bool loaded = false; // RUN_ROW of one segment: p and dp stay in LDS
    if (need_dp && (MODE == RUN_ROW || MODE == RUN_SUM)) {
        double cs = 0.0;
        for (int sg = 0; sg < nseg; ++sg) {
            const int n = min(AT_SEG, cnt - sg * AT_SEG);
            load_segment<true>(a, s, lane, q, g, e0 + (int64_t)sg * AT_SEG, n, true);
#pragma unroll
            for (int c = 0; c < AT_CELLS; ++c) {
                if (c * ROW_CELL < n) {
                    const int i = c * ROW_CELL + lane;
                    double leaf = 0.0;
                    if (i < n) {
                        const double p = fwd_out(s.sc[i], m, z);
                        s.sc[i] = p;
                        leaf = fma(p, s.dp[i], 0.0);
                    }
                    const double sum = fold_sum<64>(leaf);
                    if (lane == sg * AT_CELLS + c) cs = sum;
                }
            }
        }
        D = fold_sum<64>(cs);
        if (MODE == RUN_SUM) return;
        loaded = MODE == RUN_ROW && nseg == 1;
    }
    o0 = o1 = 0.0;
    for (int sg = 0; sg < nseg; ++sg) {
        const int n = min(AT_SEG, cnt - sg * AT_SEG);
        const int64_t base = e0 + (int64_t)sg * AT_SEG;
        if (!loaded) load_segment<true>(a, s, lane, q, g, base, n, need_dp);
#pragma unroll
        for (int c = 0; c < AT_CELLS; ++c) {
            const int i = c * ROW_CELL + lane;
            if (i < n) {
                const double p = loaded ? s.sc[i] : fwd_out(s.sc[i], m, z);
                if (a.P) a.P[base + i] = p;
                if (need_dp) {
                    const double ds = bwd_out(p, s.dp[i], D, a.scale);
                    if (a.dS) a.dS[base + i] = ds;
                    s.sc[i] = ds;
                }
            }
        }
        if (a.O) {
            __syncthreads();
            accumulate(s.sc, s.cl, n, a.K, a.ldk, a.d, a.wshift, lane, o0, o1);
        }
    }
    o0 = fold_groups(o0, a.wshift), o1 = fold_groups(o1, a.wshift);
}

// columns lane % W and lane % W + 64 of a row, written by the lanes of group 0
__device__ __forceinline__ void store_row(double *row, int ncol, int wshift, int lane, double o0, double o1)
{
    if (lane >> wshift) return;
    if (lane < ncol) row[lane] = o0;
    if (lane + 64 < ncol) row[lane + 64] = o1;
}

template <bool BWD> __global__ __launch_bounds__(AT_THREADS) void attn_rows_kernel(const Args a)
{
    __shared__ Lds<BWD> s;
    const int lane = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * AT_ROWS;
    for (int64_t r = r0; r < r0 + AT_ROWS && r < a.rows; ++r) {
        const int beg = a.rowptr[r], cnt = a.rowptr[r + 1] - beg;
        if (cnt > ROW_SUPER) continue; // the long kernels
        double m = 0.0, z = 0.0, o0 = 0.0, o1 = 0.0;
        if constexpr (BWD) {
            double D = 0.0;
            if (cnt > 0) {
                m = a.row_max[r], z = a.row_sum[r];
                backward_run<RUN_ROW>(a, s, lane, r, beg, cnt, m, z, D, o0, o1);
            }
            if (a.O) store_row(a.O + r * a.ldo, a.wn, a.wshift, lane, o0, o1);
        } else {
            forward_run<RUN_ROW>(a, s, lane, r, beg, cnt, m, z, o0, o1); // an empty row: m = -Inf, z = +0, a +0 row
            store_row(a.O + r * a.ldo, a.wn, a.wshift, lane, o0, o1);
            if (a.row_max && lane == 0) a.row_max[r] = m, a.row_sum[r] = z;
        }
    }
}

// PHASE, forward: RUN_MAX -> pmax[slot]; RUN_SUM -> psum[slot]; RUN_OUT -> part[slot]; FOLD: the first supercell's owner
// adds the row's partial rows and writes O, row_max, row_sum.  Backward: RUN_SUM -> psum[slot] (D); RUN_OUT; FOLD -> dQ.
enum { RUN_FOLD = 4 };
template <bool BWD, int PHASE> __global__ __launch_bounds__(AT_THREADS) void attn_long_kernel(const Args a)
{
    __shared__ Lds<BWD> s;
    const int lane = threadIdx.x;
    const int64_t e_first = (int64_t)blockIdx.x * ROW_SUPER;
    const int64_t e_last = e_first + ROW_SUPER - 1 < a.nnz ? e_first + ROW_SUPER - 1 : (int64_t)a.nnz - 1;
    const int r_a = block_row_of<AT_THREADS>(a.rowptr, a.rows, (int)e_first);
    const int r_b = block_row_of<AT_THREADS>(a.rowptr, a.rows, (int)e_last);
    for (int which = 0; which < 2; ++which) {
        if (which == 1 && r_b == r_a) break;
        const int r = which ? r_b : r_a;
        const int64_t row_beg = a.rowptr[r], len = (int64_t)a.rowptr[r + 1] - row_beg;
        if (len <= ROW_SUPER) continue;
        const int64_t k = row_beg >= e_first ? 0 : (e_first - row_beg + ROW_SUPER - 1) / ROW_SUPER;
        const int64_t p = row_beg + k * ROW_SUPER; // first entry of the supercell that can start in this block
        if (p > e_last || p >= row_beg + len) continue;
        const int cnt = (int)(row_beg + len - p < ROW_SUPER ? row_beg + len - p : ROW_SUPER);
        const int64_t slot = supercell_slot(row_beg, p);
        const int64_t nsuper = (len + ROW_SUPER - 1) / ROW_SUPER;
        if (PHASE == RUN_FOLD && p != row_beg) continue;

        double m = NEG_INF, z = 0.0, o0 = 0.0, o1 = 0.0;
        if constexpr (BWD) {
            m = a.row_max[r], z = a.row_sum[r];
        } else if (PHASE != RUN_MAX) { // the row's max, from the maxima of its supercells
            for (int64_t q = lane; q < nsuper; q += AT_THREADS) m = nmax(m, a.pmax[supercell_slot(row_beg, row_beg + q * ROW_SUPER)]);
            m = fold_max<64>(m);
        }
        double tot = 0.0; // the supercell sums (forward: z, backward: D), left to right
        if ((PHASE == RUN_OUT || PHASE == RUN_FOLD) && !(BWD && (PHASE == RUN_FOLD || !(a.O || a.dS)))) // backward, P alone: no D
            for (int64_t q = 0; q < nsuper; ++q) tot += a.psum[supercell_slot(row_beg, row_beg + q * ROW_SUPER)];

        if constexpr (PHASE == RUN_MAX) {
            forward_run<RUN_MAX>(a, s, lane, r, p, cnt, m, z, o0, o1);
            if (lane == 0) a.pmax[slot] = m;
        } else if constexpr (PHASE == RUN_SUM) {
            double part = 0.0;
            if constexpr (BWD) backward_run<RUN_SUM>(a, s, lane, r, p, cnt, m, z, part, o0, o1);
            else forward_run<RUN_SUM>(a, s, lane, r, p, cnt, m, part, o0, o1);
            if (lane == 0) a.psum[slot] = part;
        } else if constexpr (PHASE == RUN_OUT) {
            if constexpr (BWD) backward_run<RUN_OUT>(a, s, lane, r, p, cnt, m, z, tot, o0, o1);
            else forward_run<RUN_OUT>(a, s, lane, r, p, cnt, m, tot, o0, o1);
            if (a.O) store_row(a.part + slot * a.wpart, a.wn, a.wshift, lane, o0, o1);
        } else { // RUN_FOLD
            for (int c = lane; c < a.wn; c += AT_THREADS) {
                double acc = 0.0;
                for (int64_t q = 0; q < nsuper; ++q) acc += a.part[supercell_slot(row_beg, row_beg + q * ROW_SUPER) * a.wpart + c];
                a.O[(int64_t)r * a.ldo + c] = acc;
            }
            if (!BWD && a.row_max && lane == 0) a.row_max[r] = m, a.row_sum[r] = tot;
        }
    }
}

int64_t attn_slots(int64_t nnz) { return 2 * ((nnz + ROW_SUPER - 1) / ROW_SUPER) + 2; }

template <bool BWD> hipError_t launch_attention(hipStream_t st, Args &a, void *workspace)
{
    const unsigned grid = (unsigned)(((int64_t)a.rows + AT_ROWS - 1) / AT_ROWS);
    hipLaunchKernelGGL((attn_rows_kernel<BWD>), dim3(grid), dim3(AT_THREADS), 0, st, a);
    if (a.nnz > ROW_SUPER) { // a row longer than a supercell is possible
        const int64_t slots = attn_slots(a.nnz);
        a.pmax = static_cast<double *>(workspace), a.psum = a.pmax + slots, a.part = a.psum + slots;
        const unsigned lgrid = (unsigned)(((int64_t)a.nnz + ROW_SUPER - 1) / ROW_SUPER);
#define AT_LONG(PHASE) hipLaunchKernelGGL((attn_long_kernel<BWD, PHASE>), dim3(lgrid), dim3(AT_THREADS), 0, st, a)
        if constexpr (BWD) {
            if (a.O || a.dS) AT_LONG(RUN_SUM);
            AT_LONG(RUN_OUT);
            if (a.O) AT_LONG(RUN_FOLD);
        } else {
            AT_LONG(RUN_MAX);
            AT_LONG(RUN_SUM);
            AT_LONG(RUN_OUT);
            AT_LONG(RUN_FOLD);
        }
#undef AT_LONG
    }
    return hipGetLastError();
}

bool vec_ok(const double *x, int64_t ldx, const double *y, int64_t ldy) { return aligned16(x) && aligned16(y) && ldx % 2 == 0 && ldy % 2 == 0; }

// the checks both entry points share, before anything touches the device; SBLAS_OK with *go = false: nothing to do
int attention_args(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz, const int32_t *rowptr, const int32_t *colidx,
                   const double *Q, int64_t ldq, const double *K, int64_t ldk, const double *V, int64_t ldv, int64_t d, int64_t dv,
                   void *workspace, size_t workspace_bytes, bool *go)
{
    *go = false;
    if (rows < 0 || cols < 0 || nnz < 0 || rows > INT_MAX - 64 || cols > INT_MAX || nnz > INT_MAX || !rowptr) return SBLAS_E_INVALID;
    if (d < 1 || d > AT_MAXW || dv < 1 || dv > AT_MAXW) return SBLAS_E_INVALID;
    if (ldq < d || ldk < d || ldv < dv) return SBLAS_E_INVALID;
    if (rows > 0 && !Q) return SBLAS_E_INVALID;
    if (nnz > 0 && (!colidx || !K || !V || rows == 0 || cols == 0)) return SBLAS_E_INVALID;
    const size_t need = sblas_hip_csr_attention_workspace(rows, nnz, d, dv);
    if (need > 0 && (!workspace || workspace_bytes < need)) return SBLAS_E_WORKSPACE;
    if (need > 0 && !aligned16(workspace)) return SBLAS_E_INVALID;
    if (rows == 0) return SBLAS_OK;
    if (nnz > 0 && sblas::options().validate)
        if (const int vrc = sblas_hip_debug_validate_csr_i32(dev, stream, rows, cols, nnz, rowptr, colidx)) return vrc;
    *go = true;
    return SBLAS_OK;
}

} // namespace
} // namespace sblas

// ---- C ABI ---------------------------------------------------------------------------------------------------------
extern "C" {

size_t sblas_hip_csr_attention_workspace(int64_t rows, int64_t nnz, int64_t d, int64_t dv)
{
    if (rows <= 0 || nnz <= sblas::ROW_SUPER || d <= 0 || dv <= 0) return 0; // no row can be longer than a supercell
    const size_t w = (size_t)(d > dv ? d : dv);                               // forward and backward may share it
    return ((size_t)sblas::attn_slots(nnz) * (2 + w) * sizeof(double) + 15) / 16 * 16;
}

int sblas_hip_csr_attention_f64_i32(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz, const int32_t *rowptr,
                                    const int32_t *colidx, const double *Q, int64_t ldq, const double *K, int64_t ldk,
                                    const double *V, int64_t ldv, int64_t d, int64_t dv, double scale, double *O, int64_t ldo,
                                    double *row_max, double *row_sum, void *workspace, size_t workspace_bytes)
{
    using namespace sblas;
    if ((row_max == nullptr) != (row_sum == nullptr)) return SBLAS_E_INVALID;
    if (rows > 0 && !O) return SBLAS_E_INVALID;
    if (ldo < dv) return SBLAS_E_INVALID;
    bool go;
    if (const int rc = attention_args(dev, stream, rows, cols, nnz, rowptr, colidx, Q, ldq, K, ldk, V, ldv, d, dv, workspace,
                                      workspace_bytes, &go))
        return rc;
    if (!go) return SBLAS_OK;
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    Args a = {};
    a.rows = (int)rows, a.nnz = (int)nnz, a.rowptr = rowptr, a.colidx = colidx;
    a.Q = Q, a.K = K, a.V = V, a.ldq = ldq, a.ldk = ldk, a.ldv = ldv, a.d = (int)d, a.dv = (int)dv;
    a.gd = sddmm_group_shift(d), a.gv = sddmm_group_shift(dv), a.wshift = width_shift(dv), a.wn = (int)dv;
    a.vec_qk = vec_ok(Q, ldq, K, ldk), a.scale = scale;
    a.O = O, a.ldo = ldo, a.row_max = row_max, a.row_sum = row_sum, a.wpart = (int)(d > dv ? d : dv);
    return launch_attention<false>((hipStream_t)stream, a, workspace) == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

int sblas_hip_csr_attention_backward_f64_i32(int dev, void *stream, int64_t rows, int64_t cols, int64_t nnz, const int32_t *rowptr,
                                             const int32_t *colidx, const double *Q, int64_t ldq, const double *K, int64_t ldk,
                                             const double *V, int64_t ldv, int64_t d, int64_t dv, double scale, const double *dO,
                                             int64_t lddo, const double *row_max, const double *row_sum, double *dQ, int64_t lddq,
                                             double *P, double *dS, void *workspace, size_t workspace_bytes)
{
    using namespace sblas;
    const bool need_dp = dQ || dS;
    if (rows > 0 && (!row_max || !row_sum)) return SBLAS_E_INVALID;
    if (need_dp && ((rows > 0 && !dO) || lddo < dv)) return SBLAS_E_INVALID;
    if (dQ && lddq < d) return SBLAS_E_INVALID;
    bool go;
    if (const int rc = attention_args(dev, stream, rows, cols, nnz, rowptr, colidx, Q, ldq, K, ldk, V, ldv, d, dv, workspace,
                                      workspace_bytes, &go))
        return rc;
    if (!go || (!dQ && !P && !dS)) return SBLAS_OK; // nothing asked for
    DeviceScope scope(dev);
    if (scope.err != hipSuccess) return SBLAS_E_HIP;
    Args a = {};
    a.rows = (int)rows, a.nnz = (int)nnz, a.rowptr = rowptr, a.colidx = colidx;
    a.Q = Q, a.K = K, a.V = V, a.dO = dO, a.ldq = ldq, a.ldk = ldk, a.ldv = ldv, a.lddo = lddo, a.d = (int)d, a.dv = (int)dv;
    a.gd = sddmm_group_shift(d), a.gv = sddmm_group_shift(dv), a.wshift = width_shift(d), a.wn = (int)d;
    a.vec_qk = vec_ok(Q, ldq, K, ldk), a.vec_ov = need_dp && vec_ok(dO, lddo, V, ldv), a.scale = scale;
    a.O = dQ, a.ldo = lddq, a.row_max = const_cast<double *>(row_max), a.row_sum = const_cast<double *>(row_sum);
    a.P = P, a.dS = dS, a.wpart = (int)(d > dv ? d : dv);
    return launch_attention<true>((hipStream_t)stream, a, workspace) == hipSuccess ? SBLAS_OK : SBLAS_E_HIP;
}

} // extern "C"
