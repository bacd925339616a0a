// spmv_kernels.hip -- hand-written gfx950 (wave64) CSR SpMV kernels  y = alpha*A*x + beta*y  (replaces cusparseSpMV,
// spmv.h:104-106).  The launcher at the end takes the kernel that the kernel rule (spmv_kind, spmv_plan.cpp) picks by
// row-length class; the SpMV plan classifies its tiles by the same rule.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "kernels.h"

namespace sblas {

constexpr int WAVE = 64;
__device__ __forceinline__ int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// ---------------------------------------------------------------------------------------------
// SpMV: LPR lanes per row (a power of two, 4..64), 256/LPR rows per workgroup.  The lanes of a
// group stride through the row's nonzeros (coalesced col_idx / val streams, x gathered through
// L2), then the partial sums are folded with xor-shuffles inside the wave -- the wave64 successor of
// the reference's unused sum_32_shfl (utility.h:241-246).
// ---------------------------------------------------------------------------------------------
// The kernels below are written as a body over the block's rows [row_begin, row_end) and two entry points: the
// unplanned one derives that range from blockIdx.x (as it always has), the planned one reads it from its work item
// (sblas_hip_spmv_plan_*: int4 {first row, row count, window lo, window hi}).
template <int LPR>
__device__ __forceinline__ void spmv_csr_body(int row_begin, int row_end, const int *__restrict__ rowptr,
                                              const int *__restrict__ colidx, const double *__restrict__ val,
                                              const double *__restrict__ x, double alpha, double beta,
                                              double *__restrict__ y)
{
    constexpr int ROWS_PER_BLOCK = 256 / LPR;
    // a row far longer than the lane group was sized for (skewed matrices: the kernel is picked by the AVERAGE row
    // length) would keep its LPR lanes busy for thousands of trips while the chip idles: such rows are set aside and
    // summed by the whole block afterwards, 256 lanes striding through them
    constexpr int LONG = 64 * LPR;
    __shared__ int long_rows[ROWS_PER_BLOCK];
    __shared__ int n_long;
    __shared__ double wsum[4];
    if (threadIdx.x == 0) n_long = 0;
    __syncthreads();
    const int l = threadIdx.x % LPR;
    const int row = row_begin + threadIdx.x / LPR;
    double s0 = 0.0, s1 = 0.0;
    bool deferred = false;
    if (row < row_end) {
        const int p1 = rowptr[row + 1];
        int p = rowptr[row];
        deferred = p1 - p > LONG;
        if (deferred) {
            if (l == 0) long_rows[atomicAdd(&n_long, 1)] = row;
            p = p1;
        }
        p += l;
        // two slices per trip (four gave fewer resident waves and ran 20 % slower)
        for (; p + LPR < p1; p += 2 * LPR) {
            const int c0 = colidx[p], c1 = colidx[p + LPR];
            const double a0 = val[p], a1 = val[p + LPR];
            s0 = fma(a0, x[c0], s0);
            s1 = fma(a1, x[c1], s1);
        }
        if (p < p1) s0 = fma(val[p], x[colidx[p]], s0);
    }
    double s = s0 + s1;
#pragma unroll
    for (int m = LPR / 2; m > 0; m >>= 1) s += __shfl_xor(s, m, WAVE);
    if (row < row_end && l == 0 && !deferred) {
        const double r = alpha * s;
        y[row] = (beta == 0.0) ? r : fma(beta, y[row], r);
    }
    __syncthreads();
    for (int i = 0; i < n_long; ++i) { // (block-uniform; zero trips for all but a few blocks)
        const int lr = long_rows[i];
        const int p0 = rowptr[lr], p1 = rowptr[lr + 1];
        double t0 = 0.0, t1 = 0.0;
        int p = p0 + (int)threadIdx.x;
        for (; p + 256 < p1; p += 512) {
            const int c0 = colidx[p], c1 = colidx[p + 256];
            const double a0 = val[p], a1 = val[p + 256];
            t0 = fma(a0, x[c0], t0);
            t1 = fma(a1, x[c1], t1);
        }
        if (p < p1) t0 = fma(val[p], x[colidx[p]], t0);
        double t = t0 + t1;
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) t += __shfl_xor(t, m, WAVE);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = t;
        __syncthreads();
        if (threadIdx.x == 0) {
            const double r = alpha * (wsum[0] + wsum[1] + wsum[2] + wsum[3]);
            y[lr] = (beta == 0.0) ? r : fma(beta, y[lr], r);
        }
        __syncthreads();
    }
}
template <int LPR>
__global__ __launch_bounds__(256) void spmv_csr_kernel(int rows, const int *__restrict__ rowptr,
                                                      const int *__restrict__ colidx,
                                                      const double *__restrict__ val,
                                                      const double *__restrict__ x, double alpha, double beta,
                                                      double *__restrict__ y)
{
    spmv_csr_body<LPR>(blockIdx.x * (256 / LPR), rows, rowptr, colidx, val, x, alpha, beta, y);
}
template <int LPR>
__global__ __launch_bounds__(256) void spmv_csr_planned_kernel(const int4 *__restrict__ items, const int *__restrict__ rowptr,
                                                              const int *__restrict__ colidx,
                                                              const double *__restrict__ val,
                                                              const double *__restrict__ x, double alpha, double beta,
                                                              double *__restrict__ y)
{
    const int4 it = items[blockIdx.x];
    spmv_csr_body<LPR>(it.x, it.x + it.y, rowptr, colidx, val, x, alpha, beta, y);
}

// ---------------------------------------------------------------------------------------------
// SpMV for short and medium rows (5..64 nonzeros per row on average), stream form.  The lanes-per-row kernel gives every row a lane group
// of 4..32 lanes: a 5-nonzero row keeps 4 of 8 lanes busy for two trips, and the stencil-like matrices that have such
// rows run at 2.6-3.3 TB/s.  Here a 256-thread block owns 256 consecutive rows, i.e. ONE contiguous run of nonzeros:
// all threads stream it (thread t takes nonzeros t, t + 256, ...; every lane busy, fully coalesced), park the
// products in LDS, and thread r then adds up the products of row r in CSR order.  A block whose rows hold more than
// the LDS can take (longer rows among the short ones) takes its rows in several runs.
// ---------------------------------------------------------------------------------------------
// ST_ROWS rows per block (kernels.h).  ST_CAP = products per block held in LDS: 6144 (48 KiB + skew: three blocks per CU) or
// 4096 (33 KiB: four).  A block walks its 256 rows in runs of up to ST_CAP products, and a block in its summing phase issues
// no loads, so what pays is the fewest runs first and the most blocks per CU second (round 3; 1 M banded rows of 7 / 13 /
// 27 per row: 29.5 / 43.6 / 97.1 us with 6144 against 24.2 / 36.6 / 82 us with 4096; 600 k rows of 48, three runs instead
// of two: 128 against 141 us): the kernel rule picks per call from the average row length (spmv_kind).
constexpr int ST_LONG = 96;  // rows longer than this are summed by a whole wave
__device__ __forceinline__ int st_skew(int q) { return q + (q >> 5); } // rows of equal length: spread the LDS banks
template <int ST_CAP>
__device__ __forceinline__ void spmv_csr_stream_body(int row0, int nr, const int *__restrict__ rowptr,
                                                     const int *__restrict__ colidx, const double *__restrict__ val,
                                                     const double *__restrict__ x, double alpha, double beta,
                                                     double *__restrict__ y)
{
    __shared__ double prod[ST_CAP + ST_CAP / 32 + 1];
    __shared__ int sp[ST_ROWS + 1];
    const int tid = threadIdx.x;
    if (tid < nr) sp[tid] = rowptr[row0 + tid];
    if (tid == 0) sp[nr] = rowptr[row0 + nr];
    __syncthreads();
    __shared__ double wsum[ST_ROWS / 64];
    // The block's rows are taken in runs whose nonzeros fit the LDS: normally one run (all 256 rows); a block with
    // longer rows takes several, and a single row beyond the capacity is summed by the whole block.
    for (int r0 = 0; r0 < nr;) {
        const int base = sp[r0];
        int r1 = nr;
        if (sp[nr] - base > ST_CAP) { // largest r1 with sp[r1] - base <= ST_CAP (block-uniform: every thread searches)
            int lo = r0, hi = nr;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (sp[mid] - base <= ST_CAP) lo = mid; else hi = mid - 1;
            }
            r1 = lo;
        }
        if (r1 == r0) { // one row longer than the LDS capacity
            double sum = 0.0;
            for (int p = base + tid; p < sp[r0 + 1]; p += ST_ROWS) sum = fma(val[p], x[colidx[p]], sum);
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) sum += __shfl_xor(sum, m, WAVE);
            if ((tid & 63) == 0) wsum[tid >> 6] = sum;
            __syncthreads();
            if (tid == 0) {
                double t = 0.0;
#pragma unroll
                for (int w = 0; w < ST_ROWS / 64; ++w) t += wsum[w];
                const double res = alpha * t;
                y[row0 + r0] = (beta == 0.0) ? res : fma(beta, y[row0 + r0], res);
            }
            __syncthreads();
            r0 += 1;
            continue;
        }
        const int total = sp[r1] - base;
        // UN nonzeros per thread in flight (clamped indices instead of predicates: no waits between the loads)
        constexpr int UN = 8;
        const int lastp = max(total - 1, 0);
        for (int p = tid; p < total; p += UN * ST_ROWS) {
            int c[UN];
            double a[UN], xv[UN];
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                const int q = min(p + u * ST_ROWS, lastp);
                c[u] = colidx[base + q];
                a[u] = val[base + q];
            }
#pragma unroll
            for (int u = 0; u < UN; ++u) xv[u] = x[c[u]];
#pragma unroll
            for (int u = 0; u < UN; ++u)
                if (p + u * ST_ROWS < total) prod[st_skew(p + u * ST_ROWS)] = a[u] * xv[u];
        }
        __syncthreads();
        // thread r adds up row r in CSR order -- unless the row is long (skewed matrices: one thread walking a
        // 5000-entry row holds the whole block for ~150 us): those are summed by the 64 lanes of the row's wave
        const bool mine = tid >= r0 && tid < r1;
        const int q0 = mine ? sp[tid] - base : 0, q1 = mine ? sp[tid + 1] - base : 0;
        const bool longrow = q1 - q0 > ST_LONG;
        if (mine && !longrow) {
            double sum = 0.0;
            for (int q = q0; q < q1; ++q) sum += prod[st_skew(q)];
            const double res = alpha * sum;
            y[row0 + tid] = (beta == 0.0) ? res : fma(beta, y[row0 + tid], res);
        }
        for (unsigned long long lm = __builtin_amdgcn_ballot_w64(longrow); lm; lm &= lm - 1) {
            const int src = __builtin_ctzll(lm);                 // lane whose row this is
            const int a = __shfl(q0, src, WAVE), b = __shfl(q1, src, WAVE);
            double sum = 0.0;
            for (int q = a + (tid & 63); q < b; q += WAVE) sum += prod[st_skew(q)];
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) sum += __shfl_xor(sum, m, WAVE);
            if ((tid & 63) == src) {
                const double res = alpha * sum;
                y[row0 + tid] = (beta == 0.0) ? res : fma(beta, y[row0 + tid], res);
            }
        }
        if (r1 < nr) __syncthreads(); // prod is reused by the next run
        r0 = r1;
    }
}
template <int ST_CAP>
__global__ __launch_bounds__(ST_ROWS) void spmv_csr_stream_kernel(int rows, const int *__restrict__ rowptr,
                                                                 const int *__restrict__ colidx,
                                                                 const double *__restrict__ val,
                                                                 const double *__restrict__ x, double alpha, double beta,
                                                                 double *__restrict__ y)
{
    const int row0 = blockIdx.x * ST_ROWS;
    spmv_csr_stream_body<ST_CAP>(row0, min(ST_ROWS, rows - row0), rowptr, colidx, val, x, alpha, beta, y);
}
template <int ST_CAP>
__global__ __launch_bounds__(ST_ROWS) void spmv_csr_stream_planned_kernel(const int4 *__restrict__ items,
                                                                         const int *__restrict__ rowptr,
                                                                         const int *__restrict__ colidx,
                                                                         const double *__restrict__ val,
                                                                         const double *__restrict__ x, double alpha,
                                                                         double beta, double *__restrict__ y)
{
    const int4 it = items[blockIdx.x];
    spmv_csr_stream_body<ST_CAP>(it.x, it.y, rowptr, colidx, val, x, alpha, beta, y);
}

// ---------------------------------------------------------------------------------------------
// SpMV for medium rows (49..96 nonzeros), segmented form.  With one row per wave a 73-nonzero row (Queen_4147) fills
// 57 % of two 64-lane slices and walks two dependent trips: 2.3 TB/s.  Here a wave owns R consecutive rows -- one
// contiguous run of nonzeros -- and streams it in unpredicated slices of 64 (clamped indices, S slices in flight:
// 91 % of the lanes busy for R = 4, S = 5 at 73 per row); every lane knows the row of its entry from the R + 1 row
// pointers (wave-uniform after a readlane), products are accumulated per row and folded once at the end: the
// wave-level segmented reduction of the north star.
// ---------------------------------------------------------------------------------------------
template <int R, int S>
__global__ __launch_bounds__(256) void spmv_csr_seg_kernel(int rows, const int *__restrict__ rowptr,
                                                          const int *__restrict__ colidx,
                                                          const double *__restrict__ val,
                                                          const double *__restrict__ x, double alpha, double beta,
                                                          double *__restrict__ y)
{
    static_assert(R >= 1 && R <= 16, "row pointers are broadcast from the first R + 1 lanes");
    const int lane = threadIdx.x & 63;
    const int r0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * R;
    if (r0 >= rows) return;
    const int mine = rowptr[min(r0 + min(lane, R), rows)];
    int b[R + 1];
#pragma unroll
    for (int i = 0; i <= R; ++i) b[i] = __builtin_amdgcn_readlane(mine, i);
    const int p0 = b[0], p1 = b[R], last = p1 - 1;
    double acc[R];
#pragma unroll
    for (int i = 0; i < R; ++i) acc[i] = 0.0;
    for (int base = p0; base < p1; base += S * WAVE) {
        int c[S];
        double a[S], xv[S];
#pragma unroll
        for (int u = 0; u < S; ++u) {
            const int p = min(base + u * WAVE + lane, last);
            c[u] = colidx[p];
            a[u] = val[p];
        }
#pragma unroll
        for (int u = 0; u < S; ++u) xv[u] = x[c[u]];
#pragma unroll
        for (int u = 0; u < S; ++u) {
            const int idx = base + u * WAVE + lane;
            const double prod = (idx <= last) ? a[u] * xv[u] : 0.0;
#pragma unroll
            for (int i = 0; i < R; ++i) acc[i] += (idx >= b[i] && idx < b[i + 1]) ? prod : 0.0;
        }
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
        double sum = acc[i];
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) sum += __shfl_xor(sum, m, WAVE);
        if (lane == i && r0 + i < rows) {
            const double res = alpha * sum;
            y[r0 + i] = (beta == 0.0) ? res : fma(beta, y[r0 + i], res);
        }
    }
}

// The planned form: the same code on the rows of its work item.  (Its own copy: written as one body called by both
// kernels, the compiler gave the <4, 5> instantiation other register allocation -- 40 instead of 52 VGPRs -- and the planned
// kernel ran 16 % slower on Queen-like rows.)
template <int R, int S>
__global__ __launch_bounds__(256) void spmv_csr_seg_planned_kernel(const int4 *__restrict__ items, const int *__restrict__ rowptr,
                                                          const int *__restrict__ colidx,
                                                          const double *__restrict__ val,
                                                          const double *__restrict__ x, double alpha, double beta,
                                                          double *__restrict__ y)
{
    static_assert(R >= 1 && R <= 16, "row pointers are broadcast from the first R + 1 lanes");
    const int lane = threadIdx.x & 63;
    const int4 it = items[blockIdx.x];
    const int rows = it.x + it.y; // the end of the item's rows
    const int r0 = it.x + (int)(threadIdx.x >> 6) * R;
    if (r0 >= rows) return;
    const int mine = rowptr[min(r0 + min(lane, R), rows)];
    int b[R + 1];
#pragma unroll
    for (int i = 0; i <= R; ++i) b[i] = __builtin_amdgcn_readlane(mine, i);
    const int p0 = b[0], p1 = b[R], last = p1 - 1;
    double acc[R];
#pragma unroll
    for (int i = 0; i < R; ++i) acc[i] = 0.0;
    for (int base = p0; base < p1; base += S * WAVE) {
        int c[S];
        double a[S], xv[S];
#pragma unroll
        for (int u = 0; u < S; ++u) {
            const int p = min(base + u * WAVE + lane, last);
            c[u] = colidx[p];
            a[u] = val[p];
        }
#pragma unroll
        for (int u = 0; u < S; ++u) xv[u] = x[c[u]];
#pragma unroll
        for (int u = 0; u < S; ++u) {
            const int idx = base + u * WAVE + lane;
            const double prod = (idx <= last) ? a[u] * xv[u] : 0.0;
#pragma unroll
            for (int i = 0; i < R; ++i) acc[i] += (idx >= b[i] && idx < b[i + 1]) ? prod : 0.0;
        }
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
        double sum = acc[i];
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) sum += __shfl_xor(sum, m, WAVE);
        if (lane == i && r0 + i < rows) {
            const double res = alpha * sum;
            y[r0 + i] = (beta == 0.0) ? res : fma(beta, y[r0 + i], res);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// SpMV for long rows, x window in LDS (second attempt).  Diagnostics on the plain kernel: the A stream alone runs at
// 6.8 TB/s with the same row-per-wave shape (tools/stream_bench.hip), replacing the gather by a one-line read still
// leaves 76 us -- what costs is the second, dependent vector-memory access per slice (address unit ~15 cycles per
// instruction, more for a 40-line gather).  Here an 8-row block (one row per wave; 16 rows in round 2) fetches the x range its rows span
// into LDS once and gathers from there; the stream loads of a row (up to 448 nonzeros) are issued right after its row
// pointers, BEFORE the window is known, so the block-wide min/max, the window load and their three barriers hide
// behind the HBM latency of the stream (the barriers are `s_barrier` without the vmcnt(0) of __syncthreads).
// Columns outside the window (unsorted rows) are fetched from global memory lane by lane.
// ---------------------------------------------------------------------------------------------
// Eight waves per block and 36 KiB of window: FOUR blocks per CU, each in another phase of its life (row pointers, stream
// in flight, window fetch, gathers, reduction), so that the CU's HBM requests do not come in two bursts.  Sixteen waves and
// 40 KiB (two blocks per CU, round 2): bench matrix 68.3 us against 63.5-64.1 us now; 600 k banded rows of 160 / 260: 345 /
// 489 us against 337 / 470; 300 k rows of 500 over +-3000 (span beyond the window either way): 529 against 489.
constexpr int SPMV_LDS_THREADS = SPMV_LDS_ROWS * 64; // a wave per row of the block (kernels.h)
constexpr int SPMV_LDS_CAP = 4608;  // doubles (36 KiB): four blocks per CU
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// RW rows per wave (8 RW rows per block), S slices of 64 nonzeros fetched ahead per row.  PLANNED: the block's column
// window (plo, phi: first and last column its rows refer to) comes from the plan instead of the block-wide vote.
template <int RW, int S, bool PLANNED>
__device__ __forceinline__ void spmv_csr_lds_body(int blk, int rows, int cols, const int *__restrict__ rowptr,
                                                  const int *__restrict__ colidx, const double *__restrict__ val,
                                                  const double *__restrict__ x, double alpha, double beta,
                                                  double *__restrict__ y, int plo, int phi)
{ // blk: the block's first row in units of RW rows; rows: the end of the block's rows
    extern __shared__ __attribute__((aligned(16))) double xs[];
    __shared__ int sm_lo, sm_hi;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = wave_uniform(tid >> 6);
    const int row0 = (blk + wave) * RW;
    if (!PLANNED && tid == 0) {
        sm_lo = 0x7fffffff;
        sm_hi = -1;
    }
    int p0[RW], last[RW];
    bool has[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        int a0 = 0, a1 = 0;
        if (row0 + r < rows) {
            a0 = wave_uniform(rowptr[row0 + r]);
            a1 = wave_uniform(rowptr[row0 + r + 1]);
        }
        p0[r] = a0;
        has[r] = a1 > a0;
        last[r] = max(a1 - 1, a0);
    }
    // the two ends of every row first (lane 2r: first column of row r, lane 2r+1: its last column), then the first
    // burst of the streams
    int c[RW][S];
    double a[RW][S];
    int ce = 0;
    bool ce_valid = false;
#pragma unroll
    for (int r = 0; r < RW; ++r)
        if (!PLANNED && has[r] && (lane >> 1) == r) {
            ce = colidx[(lane & 1) ? last[r] : p0[r]];
            ce_valid = true;
        }
#pragma unroll
    for (int r = 0; r < RW; ++r)
        if (has[r]) {
#pragma unroll
            for (int u = 0; u < S; ++u) {
                const int p = min(p0[r] + u * WAVE + lane, last[r]);
                c[r][u] = colidx[p];
                a[r][u] = val[p];
            }
        }
    int lo = plo, hi = phi;
    if (!PLANNED) {
        lds_barrier(); // sm_lo / sm_hi initialised
        if (ce_valid) {
            if (lane & 1) atomicMax(&sm_hi, ce);
            else atomicMin(&sm_lo, ce);
        }
        lds_barrier();
        lo = sm_lo, hi = sm_hi;
    }
    if (lo > hi) {
        lo = 0;
        hi = -1;
    }
    lo = max(lo, 0);
    hi = min(hi, cols - 1);
    // a span that does not fit is not staged at all: every gather then goes to global memory, as in the plain kernel.
    // The window starts at an even column so that it can be fetched by LDS-DMA in 16-byte pieces (x 16-byte aligned,
    // the last pair inside x); otherwise eight bytes per thread through registers.
    lo &= ~1;
    const int wlen = (hi - lo + 1 <= SPMV_LDS_CAP) ? hi - lo + 1 : 0;
    const int pairs = (wlen + 1) >> 1;
    if (wlen > 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && lo + 2 * pairs <= cols) {
        const char *src = reinterpret_cast<const char *>(x + lo);
        for (int p0 = wave * 64; p0 < pairs; p0 += SPMV_LDS_THREADS) { // (wave-uniform trip count)
            const int pr = min(p0 + lane, pairs - 1);  // clamped lanes rewrite the last pair into the slack area
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + (size_t)pr * 16),
                                             (__attribute__((address_space(3))) void *)(xs + 2 * p0), 16, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else if (wlen > 0) {
        // the whole window in one burst of loads (clamped indices), then the stores
        constexpr int PASSES = SPMV_LDS_CAP / SPMV_LDS_THREADS;
        double t[PASSES];
#pragma unroll
        for (int j = 0; j < PASSES; ++j) t[j] = x[lo + min(tid + SPMV_LDS_THREADS * j, wlen - 1)];
#pragma unroll
        for (int j = 0; j < PASSES; ++j)
            if (tid + SPMV_LDS_THREADS * j < wlen) xs[tid + SPMV_LDS_THREADS * j] = t[j];
    }
    lds_barrier();
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        const int row = row0 + r;
        if (row >= rows) break;
        double s0 = 0.0, s1 = 0.0;
        if (has[r]) {
            for (int base = p0[r];;) {
                double xv[S];
                bool out = false;
#pragma unroll
                for (int u = 0; u < S; ++u) {
                    const bool live = base + u * WAVE + lane <= last[r];
                    const unsigned rel = (unsigned)(c[r][u] - lo);
                    const bool inw = rel < (unsigned)wlen;
                    // never multiply by unstaged LDS (a block whose span is not staged has wlen = 0) nor, in a clamped
                    // lane, by a staged Inf / NaN that belongs to another entry: dead lanes contribute exactly 0 * 0
                    const double staged = xs[inw ? rel : 0u];
                    xv[u] = (inw && live) ? staged : 0.0;
                    out |= live && !inw;
                }
                if (__builtin_amdgcn_ballot_w64(out) != 0ull) { // columns outside the window (unsorted rows, wide spans)
#pragma unroll
                    for (int u = 0; u < S; ++u) {
                        const bool live = base + u * WAVE + lane <= last[r];
                        if (live && (unsigned)(c[r][u] - lo) >= (unsigned)wlen) xv[u] = x[c[r][u]];
                    }
                }
#pragma unroll
                for (int u = 0; u < S; ++u) {
                    const double av = (base + u * WAVE + lane <= last[r]) ? a[r][u] : 0.0;
                    if (u & 1) s1 = fma(av, xv[u], s1);
                    else s0 = fma(av, xv[u], s0);
                }
                base += S * WAVE;
                if (base > last[r]) break;
#pragma unroll
                for (int u = 0; u < S; ++u) {
                    const int p = min(base + u * WAVE + lane, last[r]);
                    c[r][u] = colidx[p];
                    a[r][u] = val[p];
                }
            }
        }
        double sum = s0 + s1;
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) sum += __shfl_xor(sum, m, WAVE);
        if (lane == 0) {
            const double res = alpha * sum;
            y[row] = (beta == 0.0) ? res : fma(beta, y[row], res);
        }
    }
}
template <int RW, int S>
__global__ __launch_bounds__(SPMV_LDS_THREADS) void spmv_csr_lds_kernel(int rows, int cols, const int *__restrict__ rowptr,
                                                           const int *__restrict__ colidx,
                                                           const double *__restrict__ val,
                                                           const double *__restrict__ x, double alpha, double beta,
                                                           double *__restrict__ y)
{
    spmv_csr_lds_body<RW, S, false>(blockIdx.x * SPMV_LDS_ROWS, rows, cols, rowptr, colidx, val, x, alpha, beta, y, 0, 0);
}
template <int S> // one row per wave
__global__ __launch_bounds__(SPMV_LDS_THREADS) void spmv_csr_lds_planned_kernel(const int4 *__restrict__ items, int cols,
                                                                   const int *__restrict__ rowptr,
                                                                   const int *__restrict__ colidx,
                                                                   const double *__restrict__ val,
                                                                   const double *__restrict__ x, double alpha, double beta,
                                                                   double *__restrict__ y)
{
    const int4 it = items[blockIdx.x];
    spmv_csr_lds_body<1, S, true>(it.x, it.x + it.y, cols, rowptr, colidx, val, x, alpha, beta, y, it.z, it.w);
}


// One unplanned launch: the kernels' common arguments, and a launcher per kernel form.
struct SpmvCall {
    hipStream_t s;
    int rows, cols;
    const int *rowptr, *colidx;
    const double *val, *x;
    double alpha, beta;
    double *y;
};
template <int LPR>
static hipError_t spmv_go(const SpmvCall &c)
{
    constexpr int rpb = 256 / LPR;
    hipLaunchKernelGGL(spmv_csr_kernel<LPR>, dim3((unsigned)((c.rows + rpb - 1) / rpb)), dim3(256), 0, c.s, c.rows, c.rowptr,
                       c.colidx, c.val, c.x, c.alpha, c.beta, c.y);
    return hipGetLastError();
}
template <int ST_CAP>
static hipError_t spmv_stream_go(const SpmvCall &c)
{
    hipLaunchKernelGGL(spmv_csr_stream_kernel<ST_CAP>, dim3((unsigned)((c.rows + ST_ROWS - 1) / ST_ROWS)), dim3(ST_ROWS), 0, c.s,
                       c.rows, c.rowptr, c.colidx, c.val, c.x, c.alpha, c.beta, c.y);
    return hipGetLastError();
}
template <int R, int S>
static hipError_t spmv_seg_go(const SpmvCall &c)
{
    hipLaunchKernelGGL((spmv_csr_seg_kernel<R, S>), dim3((unsigned)((c.rows + 4 * R - 1) / (4 * R))), dim3(256), 0, c.s, c.rows,
                       c.rowptr, c.colidx, c.val, c.x, c.alpha, c.beta, c.y);
    return hipGetLastError();
}
template <int RW, int S>
static hipError_t spmv_lds_go(const SpmvCall &c)
{
    raise_dynamic_lds((const void *)spmv_csr_lds_kernel<RW, S>, (SPMV_LDS_CAP + 128) * sizeof(double));
    hipLaunchKernelGGL((spmv_csr_lds_kernel<RW, S>), dim3((unsigned)((c.rows + SPMV_LDS_ROWS * RW - 1) / (SPMV_LDS_ROWS * RW))),
                       dim3(SPMV_LDS_THREADS), (SPMV_LDS_CAP + 128) * sizeof(double), c.s, c.rows, c.cols, c.rowptr, c.colidx,
                       c.val, c.x, c.alpha, c.beta, c.y);
    return hipGetLastError();
}

// the unplanned instantiation of an SBLAS_SPMV_ITEM_* kind
static hipError_t spmv_kind_go(const SpmvCall &c, int kind)
{
    switch (kind) {
    case SBLAS_SPMV_ITEM_LDS_S2: return spmv_lds_go<1, 2>(c);
    case SBLAS_SPMV_ITEM_LDS_S3: return spmv_lds_go<1, 3>(c);
    case SBLAS_SPMV_ITEM_LDS_S4: return spmv_lds_go<1, 4>(c);
    case SBLAS_SPMV_ITEM_LDS_S7: return spmv_lds_go<1, 7>(c);
    case SBLAS_SPMV_ITEM_SEG: return spmv_seg_go<SPMV_SEG_R, 5>(c);
    case SBLAS_SPMV_ITEM_STREAM4096: return spmv_stream_go<4096>(c);
    case SBLAS_SPMV_ITEM_STREAM6144: return spmv_stream_go<6144>(c);
    default: return spmv_go<SPMV_LPR>(c);
    }
}

hipError_t launch_spmv(hipStream_t s, int rows, int cols, int64_t nnz, const int *rowptr, const int *colidx,
                       const double *val, const double *x, double alpha, double beta, double *y)
{
    const SpmvCall c{s, rows, cols, rowptr, colidx, val, x, alpha, beta, y};
    const double avg = rows > 0 ? (double)nnz / (double)rows : 0.0;
    const char *sv = options().spmv_variant; // "" = auto: the kernel rule; anything else pins a kernel (A/B runs, tests)
    if (!*sv) return spmv_kind_go(c, spmv_kind(avg));
    auto is = [&](const char *name) { return !strcmp(sv, name); };
    if (is("lds")) return spmv_kind_go(c, SBLAS_SPMV_ITEM_LDS_S7);
    if (is("lds2")) return spmv_lds_go<2, 7>(c);
    if (is("lds1s2")) return spmv_kind_go(c, SBLAS_SPMV_ITEM_LDS_S2);
    if (is("lds1s3")) return spmv_kind_go(c, SBLAS_SPMV_ITEM_LDS_S3);
    if (is("lds1s4")) return spmv_kind_go(c, SBLAS_SPMV_ITEM_LDS_S4);
    if (is("seg4")) return spmv_kind_go(c, SBLAS_SPMV_ITEM_SEG);
    if (is("seg3")) return spmv_seg_go<3, 4>(c);
    if (is("seg8")) return spmv_seg_go<8, 5>(c);
    if (is("seg2")) return spmv_seg_go<2, 3>(c);
    if (is("stream")) return spmv_kind_go(c, spmv_kind(avg, SBLAS_SPMV_ITEM_STREAM4096));
    // "plain" (and anything unknown): lanes per row by average length
    if (avg <= 6.0) return spmv_go<4>(c);
    if (avg <= 12.0) return spmv_go<8>(c);
    if (avg <= 24.0) return spmv_go<16>(c);
    if (avg <= 48.0) return spmv_go<32>(c);
    return spmv_go<64>(c);
}

// ---------------------------------------------------------------------------------------------
// Split rows (planned calls only).  A row of 10^5..10^6 nonzeros in the kernels above is walked by one block (stream,
// lanes-per-row) or one wave (segmented, LDS-window) while the rest of the GPU idles.  The plan cuts such a row into
// pieces of SBLAS_SPMV_SPLIT_PIECE nonzeros, contiguous in CSR order; one 256-thread workgroup sums a piece into a
// partial of the plan's buffer, and a second kernel folds the partials of a row in piece order and applies alpha / beta.
// No atomics, no workgroup waits on another: the order of every addition is fixed by the plan, so the result is the same
// bits on every call.  Inside a piece thread t takes nonzeros t, t + 256, ... (UN loads in flight, clamped indices, as in
// the stream kernel), the 64 lanes of a wave are folded by the xor-butterfly and the four waves in wave order.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void spmv_split_piece_kernel(const int4 *__restrict__ pieces,
                                                              const int *__restrict__ colidx,
                                                              const double *__restrict__ val,
                                                              const double *__restrict__ x, double *__restrict__ partial)
{
    __shared__ double wsum[4];
    const int4 pc = pieces[blockIdx.x]; // {row, first nonzero, end, partial slot}
    const int tid = threadIdx.x;
    const int last = pc.z - 1;
    constexpr int UN = 8;
    double acc = 0.0;
    for (int p = pc.y + tid; p < pc.z; p += UN * 256) {
        int c[UN];
        double a[UN], xv[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int q = min(p + u * 256, last);
            c[u] = colidx[q];
            a[u] = val[q];
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) xv[u] = x[c[u]];
#pragma unroll
        for (int u = 0; u < UN; ++u)
            if (p + u * 256 < pc.z) acc = fma(a[u], xv[u], acc);
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) acc += __shfl_xor(acc, m, WAVE);
    if ((tid & 63) == 0) wsum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) partial[pc.w] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// one wave per split row: 64 partials loaded at a time, added in piece order by lane 0's walk through them (readlane)
__device__ __forceinline__ double readlane_f64(double v, int l)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__global__ __launch_bounds__(64) void spmv_split_fold_kernel(const int4 *__restrict__ srows, const double *__restrict__ partial,
                                                            double alpha, double beta, double *__restrict__ y)
{
    const int4 sr = srows[blockIdx.x]; // {row, first slot, pieces, -}
    const int lane = threadIdx.x;
    double sum = 0.0;
    for (int j0 = 0; j0 < sr.z; j0 += 64) {
        const double v = (j0 + lane < sr.z) ? partial[sr.y + j0 + lane] : 0.0;
        const int m = min(64, sr.z - j0);
        for (int j = 0; j < m; ++j) sum += readlane_f64(v, j);
    }
    if (lane == 0) {
        const double res = alpha * sum;
        y[sr.x] = (beta == 0.0) ? res : fma(beta, y[sr.x], res);
    }
}

// the column window of every LDS-window item (first and last column its rows refer to): the block-wide vote of the
// unplanned kernel, taken once when the plan is made
__global__ __launch_bounds__(256) void spmv_plan_window_kernel(int n, int4 *__restrict__ items, const int *__restrict__ rowptr,
                                                              const int *__restrict__ colidx)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int4 it = items[i];
    int lo = 0x7fffffff, hi = -1;
    for (int r = it.x; r < it.x + it.y; ++r) {
        const int a0 = rowptr[r], a1 = rowptr[r + 1];
        if (a1 > a0) {
            lo = min(lo, colidx[a0]);
            hi = max(hi, colidx[a1 - 1]);
        }
    }
    it.z = lo;
    it.w = hi;
    items[i] = it;
}

hipError_t spmv_plan_windows(hipStream_t s, int n, int4 *items, const int *rowptr, const int *colidx)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(spmv_plan_window_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, items, rowptr, colidx);
    return hipGetLastError();
}

// A planned call: one launch per non-empty class, in the order of the SBLAS_SPMV_ITEM_* numbers, then the split rows'
// pieces and their fold.  Every launch writes rows no other launch writes.
hipError_t launch_spmv_planned(hipStream_t s, int cols, const SpmvPlanView &pv, const int *rowptr, const int *colidx,
                               const double *val, const double *x, double alpha, double beta, double *y)
{
    auto grid = [&](int k) { return dim3((unsigned)(pv.off[k + 1] - pv.off[k])); };
    auto items = [&](int k) { return pv.items + pv.off[k]; };
    auto has = [&](int k) { return pv.off[k + 1] > pv.off[k]; };
    if (has(SBLAS_SPMV_ITEM_LPR))
        hipLaunchKernelGGL(spmv_csr_planned_kernel<SPMV_LPR>, grid(SBLAS_SPMV_ITEM_LPR), dim3(256), 0, s, items(SBLAS_SPMV_ITEM_LPR),
                           rowptr, colidx, val, x, alpha, beta, y);
    if (has(SBLAS_SPMV_ITEM_STREAM4096))
        hipLaunchKernelGGL(spmv_csr_stream_planned_kernel<4096>, grid(SBLAS_SPMV_ITEM_STREAM4096), dim3(ST_ROWS), 0, s,
                           items(SBLAS_SPMV_ITEM_STREAM4096), rowptr, colidx, val, x, alpha, beta, y);
    if (has(SBLAS_SPMV_ITEM_STREAM6144))
        hipLaunchKernelGGL(spmv_csr_stream_planned_kernel<6144>, grid(SBLAS_SPMV_ITEM_STREAM6144), dim3(ST_ROWS), 0, s,
                           items(SBLAS_SPMV_ITEM_STREAM6144), rowptr, colidx, val, x, alpha, beta, y);
    if (has(SBLAS_SPMV_ITEM_SEG))
        hipLaunchKernelGGL((spmv_csr_seg_planned_kernel<SPMV_SEG_R, 5>), grid(SBLAS_SPMV_ITEM_SEG), dim3(256), 0, s,
                           items(SBLAS_SPMV_ITEM_SEG), rowptr, colidx, val, x, alpha, beta, y);
#define SBLAS_SPMV_LDS_PLANNED(K, SV)                                                                                \
    if (has(K)) {                                                                                                    \
        raise_dynamic_lds((const void *)spmv_csr_lds_planned_kernel<SV>, (SPMV_LDS_CAP + 128) * sizeof(double));     \
        hipLaunchKernelGGL(spmv_csr_lds_planned_kernel<SV>, grid(K), dim3(SPMV_LDS_THREADS),                         \
                           (SPMV_LDS_CAP + 128) * sizeof(double), s, items(K), cols, rowptr, colidx, val, x, alpha,   \
                           beta, y);                                                                                 \
    }
    SBLAS_SPMV_LDS_PLANNED(SBLAS_SPMV_ITEM_LDS_S2, 2)
    SBLAS_SPMV_LDS_PLANNED(SBLAS_SPMV_ITEM_LDS_S3, 3)
    SBLAS_SPMV_LDS_PLANNED(SBLAS_SPMV_ITEM_LDS_S4, 4)
    SBLAS_SPMV_LDS_PLANNED(SBLAS_SPMV_ITEM_LDS_S7, 7)
#undef SBLAS_SPMV_LDS_PLANNED
    if (pv.n_pieces > 0) {
        hipLaunchKernelGGL(spmv_split_piece_kernel, dim3((unsigned)pv.n_pieces), dim3(256), 0, s, pv.pieces, colidx, val, x,
                           pv.partial);
        hipLaunchKernelGGL(spmv_split_fold_kernel, dim3((unsigned)pv.n_split), dim3(64), 0, s, pv.srows, pv.partial, alpha,
                           beta, y);
    }
    return hipGetLastError();
}

} // namespace sblas
