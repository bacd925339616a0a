// rowwise.h -- device helpers the per-entry and per-row kernels on a CSR pattern share (sddmm.hip, softmax.hip,
// attention.hip): the dot-product pieces and lane-group butterfly of SDDMM, the cell / supercell folds,
// the NaN-propagating max and the output expressions of the softmax (3.16), the 256-way search in rowptr and the
// workspace slot of a supercell.  One definition each: the kernels that promise each other's bits call the same code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sblas {

constexpr int ROW_CELL = 64;     // leaves per cell: one wave-wide butterfly
constexpr int ROW_SUPER = 4096;  // leaves per supercell: 64 cells
constexpr int SDDMM_SLICE = 128; // elements of k per SDDMM launch; the widest row the fused attention kernels take

// Lanes per nonzero for a slice of k elements, settled by measurement: a lane takes up to four elements
// of each row for k <= 16 and up to eight beyond, i.e. up to four 16-byte loads per row in flight; fewer lanes with more
// pieces each, or more lanes with one piece each, ran up to 1.4 x slower.  The order of a dot product follows from it,
// so sddmm.hip and attention.hip, which promise each other's bits, both take it from here.
constexpr int sddmm_group(int64_t k) { return k <= 4 ? 1 : k <= 8 ? 2 : k <= 32 ? 4 : k <= 64 ? 8 : 16; }
// the same as a shift: sddmm_group(k) == 1 << sddmm_group_shift(k)
constexpr int sddmm_group_shift(int64_t k) { return sddmm_group(k) == 1 ? 0 : sddmm_group(k) == 2 ? 1 : sddmm_group(k) == 4 ? 2 : sddmm_group(k) == 8 ? 3 : 4; }
static_assert(sddmm_group(SDDMM_SLICE) == 16 && 2 * 4 * sddmm_group(SDDMM_SLICE) >= SDDMM_SLICE, "four rounds of pieces cover a slice");

template <int CTRL> __device__ __forceinline__ double dpp_f64(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// The butterfly over the G lanes of a group (G lanes aligned inside a DPP row of 16).  Once the lanes of a quad hold one
// sum, the half-row mirror hands every lane the sum of the other quad of its eight (what l ^ 4 would), and the row mirror
// after it the sum of the other eight.
template <int G> __device__ __forceinline__ double group_sum(double s)
{
    if constexpr (G >= 2) s += dpp_f64<0xB1>(s);  // quad_perm:[1,0,3,2]
    if constexpr (G >= 4) s += dpp_f64<0x4E>(s);  // quad_perm:[2,3,0,1]
    if constexpr (G >= 8) s += dpp_f64<0x141>(s); // row_half_mirror
    if constexpr (G >= 16) s += dpp_f64<0x140>(s); // row_mirror
    return s;
}

// elements j, j + 1 of a row, those below k only: what is masked off is never loaded (it may lie outside the operand)
template <bool VEC, bool FULL> __device__ __forceinline__ double2 load_piece(const double *__restrict__ row, int j, int k)
{
    double2 v = make_double2(0.0, 0.0);
    if (FULL || j + 1 < k) {
        if constexpr (VEC) v = *reinterpret_cast<const double2 *>(row + j);
        else v = make_double2(row[j], row[j + 1]);
    } else if (j < k) {
        v.x = row[j];
    }
    return v;
}

// largest r in [0, rows) with rowptr[r] <= e, for 0 <= e < rowptr[rows]: the row that holds entry e.  All THREADS threads
// of the workgroup probe, log2(THREADS) bits of the answer a round
template <int THREADS> __device__ __forceinline__ int block_row_of(const int *__restrict__ rowptr, int rows, int e)
{
    int64_t lo = 0, hi = rows; // rowptr[lo] <= e < rowptr[hi]
    while (hi - lo > 1) {
        const int64_t step = (hi - lo + THREADS - 1) / THREADS;
        const int64_t p = lo + ((int64_t)threadIdx.x + 1) * step;
        const int below = (p < hi && rowptr[p] <= e) ? 1 : 0;
        const int64_t cnt = __syncthreads_count(below);
        const int64_t nlo = lo + cnt * step, nhi = lo + (cnt + 1) * step;
        lo = nlo;
        if (nhi < hi) hi = nhi;
    }
    return (int)lo;
}

// the value the lane LEVEL places away holds (l ^ LEVEL), for lanes that already agree inside their group of LEVEL: the
// quad permutes, then the half-row and row mirrors (group_sum), then lane permutes across the DPP rows
template <int LEVEL> __device__ __forceinline__ double lane_partner(double v)
{
    if constexpr (LEVEL == 1) return dpp_f64<0xB1>(v);       // quad_perm:[1,0,3,2]
    else if constexpr (LEVEL == 2) return dpp_f64<0x4E>(v);  // quad_perm:[2,3,0,1]
    else if constexpr (LEVEL == 4) return dpp_f64<0x141>(v); // row_half_mirror
    else if constexpr (LEVEL == 8) return dpp_f64<0x140>(v); // row_mirror
    else return __shfl_xor(v, LEVEL, 64);
}
// NaN wins; otherwise the larger (which zero of +0 / -0 comes back does not matter: exp(+-0) = 1)
__device__ __forceinline__ double nmax(double a, double b) { return (a > b || a != a) ? a : b; }

template <int LANES> __device__ __forceinline__ double fold_sum(double v)
{
    if constexpr (LANES >= 2) v += lane_partner<1>(v);
    if constexpr (LANES >= 4) v += lane_partner<2>(v);
    if constexpr (LANES >= 8) v += lane_partner<4>(v);
    if constexpr (LANES >= 16) v += lane_partner<8>(v);
    if constexpr (LANES >= 32) v += lane_partner<16>(v);
    if constexpr (LANES >= 64) v += lane_partner<32>(v);
    return v;
}
template <int LANES> __device__ __forceinline__ double fold_max(double v)
{
    if constexpr (LANES >= 2) v = nmax(v, lane_partner<1>(v));
    if constexpr (LANES >= 4) v = nmax(v, lane_partner<2>(v));
    if constexpr (LANES >= 8) v = nmax(v, lane_partner<4>(v));
    if constexpr (LANES >= 16) v = nmax(v, lane_partner<8>(v));
    if constexpr (LANES >= 32) v = nmax(v, lane_partner<16>(v));
    if constexpr (LANES >= 64) v = nmax(v, lane_partner<32>(v));
    return v;
}

constexpr double NEG_INF = -__builtin_huge_val();

// ---- the outputs of the softmax, the same expressions on every path; each operation is rounded on its own ------------
__device__ __forceinline__ double fwd_out(double t, double m, double s)
{
#pragma clang fp contract(off)
    return exp(t - m) / s;
}
__device__ __forceinline__ double bwd_out(double p, double dp, double d, double scale)
{
#pragma clang fp contract(off)
    return (scale * p) * (dp - d);
}

// the workspace slot of the supercell of a row (first entry row_beg) that starts at entry p: no two supercells share one
__device__ __forceinline__ int64_t supercell_slot(int64_t row_beg, int64_t p) { return 2 * (p / ROW_SUPER) + (p == row_beg ? 1 : 0); }

} // namespace sblas
