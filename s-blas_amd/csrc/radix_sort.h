// radix_sort.h -- the device pieces transpose.hip and coo.hip share: a stable LSD radix sort of int32 keys with an index
// payload (8-bit digits: histogram, three-kernel exclusive scan, ranked scatter; no atomics), the lower-bound pointer
// builder and the fp64 value gather.  transpose.hip's header comment describes the passes.  Internal to each translation
// unit: nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int T_THREADS = 256;                        // four waves
constexpr int T_WAVES = T_THREADS / 64;
constexpr int T_ROUNDS = 16;                          // keys per lane
constexpr int64_t T_WAVE_KEYS = 64 * T_ROUNDS;        // contiguous keys of one wave
constexpr int64_t T_TILE = T_WAVES * T_WAVE_KEYS;     // 4096 keys per workgroup
constexpr int RADIX_BITS = 8;
constexpr int RADIX = 1 << RADIX_BITS;
constexpr int SCAN_ITEMS = 16;
constexpr int64_t SCAN_TILE = T_THREADS * SCAN_ITEMS; // 4096 histogram entries per workgroup

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline size_t align16(size_t b) { return (b + 15) / 16 * 16; }

// bits of the largest column index, and the 8-bit passes they take (0 for one column: the CSR order is already sorted)
inline int key_bits(int64_t cols)
{
    int b = 0;
    for (uint64_t v = cols > 1 ? (uint64_t)(cols - 1) : 0; v; v >>= 1) ++b;
    return b;
}
inline int radix_passes(int64_t cols) { return (key_bits(cols) + RADIX_BITS - 1) / RADIX_BITS; }

struct Workspace {
    int32_t *keys[2] = {nullptr, nullptr}, *idx[2] = {nullptr, nullptr};
    uint32_t *hist = nullptr, *bsum = nullptr;
    int64_t tiles = 0, hist_len = 0, scan_blocks = 0;
};

// key / payload ping-pong buffers (16 B per nonzero), the digit-major histogram (1 KiB per tile) and the scan's block sums
inline size_t workspace_layout(int64_t nnz, char *base, Workspace *w)
{
    const int64_t tiles = ceil_div(nnz, T_TILE), hist_len = (int64_t)RADIX * tiles, scan_blocks = ceil_div(hist_len, SCAN_TILE);
    const size_t arr = align16((size_t)nnz * sizeof(int32_t));
    size_t off = 0;
    if (w) {
        w->tiles = tiles, w->hist_len = hist_len, w->scan_blocks = scan_blocks;
        for (int q = 0; q < 2; ++q) {
            w->keys[q] = reinterpret_cast<int32_t *>(base + off), off += arr;
            w->idx[q] = reinterpret_cast<int32_t *>(base + off), off += arr;
        }
        w->hist = reinterpret_cast<uint32_t *>(base + off), off += align16((size_t)hist_len * sizeof(uint32_t));
        w->bsum = reinterpret_cast<uint32_t *>(base + off), off += align16((size_t)scan_blocks * sizeof(uint32_t));
        return off;
    }
    return 4 * arr + align16((size_t)hist_len * sizeof(uint32_t)) + align16((size_t)scan_blocks * sizeof(uint32_t));
}

inline unsigned grid_for(int64_t n)
{
    const int64_t b = ceil_div(n, T_THREADS);
    return (unsigned)(b < 1 ? 1 : b > 65536 ? 65536 : b); // grid-stride loops cover the rest
}

// the lanes of this wave whose (valid) key has digit d, as a 64-bit lane mask; every lane of the wave must call it
__device__ inline uint64_t match_digit(uint32_t d, bool valid)
{
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < RADIX_BITS; ++b) {
        const bool bit = (d >> b) & 1u;
        const uint64_t v = __ballot(bit);
        m &= bit ? v : ~v;
    }
    return m;
}

__global__ __launch_bounds__(T_THREADS) void radix_hist_kernel(const int32_t *__restrict__ keys, int64_t nnz, int shift,
                                                               int64_t tiles, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t cnt[T_WAVES][RADIX];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    for (int q = tid; q < T_WAVES * RADIX; q += T_THREADS) (&cnt[0][0])[q] = 0;
    __syncthreads();
    const int64_t t = blockIdx.x;
    const int64_t base = t * T_TILE + (int64_t)w * T_WAVE_KEYS + lane;
    volatile uint32_t *wc = cnt[w]; // wave-private: one leader per digit and round, rounds in order
    for (int j = 0; j < T_ROUNDS; ++j) {
        const int64_t i = base + (int64_t)j * 64;
        const bool valid = i < nnz;
        const uint32_t d = valid ? ((uint32_t)keys[i] >> shift) & (RADIX - 1) : 0u;
        const uint64_t m = match_digit(d, valid);
        if (valid && lane == __ffsll((unsigned long long)m) - 1) wc[d] = wc[d] + (uint32_t)__popcll(m);
    }
    __syncthreads();
    uint32_t s = 0;
    for (int q = 0; q < T_WAVES; ++q) s += cnt[q][tid];
    hist[(int64_t)tid * tiles + t] = s;
}

__global__ __launch_bounds__(T_THREADS) void radix_scatter_kernel(const int32_t *__restrict__ keys_in,
                                                                  const int32_t *__restrict__ idx_in, int64_t nnz, int shift,
                                                                  int64_t tiles, const uint32_t *__restrict__ offs,
                                                                  int32_t *__restrict__ keys_out, int32_t *__restrict__ idx_out)
{
    __shared__ uint32_t cnt[T_WAVES][RADIX];
    __shared__ uint32_t keys[T_WAVES][T_WAVE_KEYS];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    for (int q = tid; q < T_WAVES * RADIX; q += T_THREADS) (&cnt[0][0])[q] = 0;
    __syncthreads();
    const int64_t t = blockIdx.x;
    const int64_t base = t * T_TILE + (int64_t)w * T_WAVE_KEYS + lane;
    const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
    volatile uint32_t *wc = cnt[w];
    uint32_t *wkeys = keys[w]; // the wave's keys, read once from memory
    for (int j = 0; j < T_ROUNDS; ++j) { // count this wave's digits
        const int64_t i = base + (int64_t)j * 64;
        const bool valid = i < nnz;
        const uint32_t key = valid ? (uint32_t)keys_in[i] : 0u;
        wkeys[j * 64 + lane] = key;
        const uint32_t d = (key >> shift) & (RADIX - 1);
        const uint64_t m = match_digit(d, valid);
        if (valid && lane == __ffsll((unsigned long long)m) - 1) wc[d] = wc[d] + (uint32_t)__popcll(m);
    }
    __syncthreads();
    { // a wave's first slot of digit d: the tile's base for d plus the earlier waves' keys of d
        uint32_t run = offs[(int64_t)tid * tiles + t];
        for (int q = 0; q < T_WAVES; ++q) {
            const uint32_t c = cnt[q][tid];
            cnt[q][tid] = run;
            run += c;
        }
    }
    __syncthreads();
    for (int j = 0; j < T_ROUNDS; ++j) {
        const int64_t i = base + (int64_t)j * 64;
        const bool valid = i < nnz;
        const uint32_t key = wkeys[j * 64 + lane];
        const uint32_t d = (key >> shift) & (RADIX - 1);
        const uint64_t m = match_digit(d, valid);
        if (valid) {
            const uint32_t b = wc[d]; // every lane of the group reads before its leader moves the counter on
            const uint32_t dst = b + (uint32_t)__popcll(m & below);
            keys_out[dst] = (int32_t)key;
            idx_out[dst] = idx_in ? idx_in[i] : (int32_t)i;
            if (lane == __ffsll((unsigned long long)m) - 1) wc[d] = b + (uint32_t)__popcll(m);
        }
    }
}

// exclusive prefix of v over the workgroup's 256 threads
__device__ inline uint32_t block_exclusive_scan(uint32_t v, uint32_t *total)
{
    __shared__ uint32_t wsum[T_WAVES];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    uint32_t pre = 0, all = 0;
    for (int q = 0; q < T_WAVES; ++q) {
        pre += q < w ? wsum[q] : 0u;
        all += wsum[q];
    }
    __syncthreads();
    *total = all;
    return pre + x - v;
}

__global__ __launch_bounds__(T_THREADS) void scan_reduce_kernel(const uint32_t *__restrict__ a, int64_t n, uint32_t *__restrict__ bsum)
{
    const int64_t b0 = (int64_t)blockIdx.x * SCAN_TILE;
    uint32_t s = 0;
    for (int j = 0; j < SCAN_ITEMS; ++j) {
        const int64_t i = b0 + (int64_t)j * T_THREADS + threadIdx.x;
        if (i < n) s += a[i];
    }
    uint32_t total;
    (void)block_exclusive_scan(s, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup: exclusive scan of the block sums in place
__global__ __launch_bounds__(T_THREADS) void scan_top_kernel(uint32_t *__restrict__ bsum, int64_t nb)
{
    uint32_t carry = 0;
    for (int64_t c = 0; c < nb; c += T_THREADS) {
        const int64_t i = c + threadIdx.x;
        const uint32_t v = i < nb ? bsum[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan(v, &total);
        if (i < nb) bsum[i] = carry + ex;
        carry += total;
    }
}

// exclusive scan of one tile in place (16 consecutive entries per thread), offset by the tile's block sum
__global__ __launch_bounds__(T_THREADS) void scan_down_kernel(uint32_t *__restrict__ a, int64_t n, const uint32_t *__restrict__ bsum)
{
    const int64_t i0 = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    uint32_t v[SCAN_ITEMS], s = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
        v[j] = i0 + j < n ? a[i0 + j] : 0u;
        s += v[j];
    }
    uint32_t total;
    uint32_t run = bsum[blockIdx.x] + block_exclusive_scan(s, &total);
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
        if (i0 + j < n) a[i0 + j] = run;
        run += v[j];
    }
}

// colptr[c] = number of sorted keys below c, c = 0 .. cols; with `count`, count[that number] (coo.hip: the entries before
// the first triplet of row c)
__global__ __launch_bounds__(T_THREADS) void colptr_kernel(const int32_t *__restrict__ skeys, int64_t nnz, int64_t cols,
                                                           const uint32_t *__restrict__ count, int32_t *__restrict__ colptr)
{
    for (int64_t c = (int64_t)blockIdx.x * T_THREADS + threadIdx.x; c <= cols; c += (int64_t)gridDim.x * T_THREADS) {
        int64_t lo = 0, hi = nnz;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)skeys[mid] < c) lo = mid + 1;
            else hi = mid;
        }
        colptr[c] = count ? (int32_t)count[lo] : (int32_t)lo;
    }
}

__global__ __launch_bounds__(T_THREADS) void gather_f64_kernel(int64_t n, const int32_t *__restrict__ idx,
                                                               const double *__restrict__ src, double *__restrict__ dst)
{
    for (int64_t i = (int64_t)blockIdx.x * T_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * T_THREADS) dst[i] = src[idx[i]];
}

hipError_t scan_exclusive(hipStream_t s, uint32_t *a, int64_t n, uint32_t *bsum, int64_t nb)
{
    scan_reduce_kernel<<<(unsigned)nb, T_THREADS, 0, s>>>(a, n, bsum);
    scan_top_kernel<<<1, T_THREADS, 0, s>>>(bsum, nb);
    scan_down_kernel<<<(unsigned)nb, T_THREADS, 0, s>>>(a, n, bsum);
    return hipGetLastError();
}

// one stable pass on the 8-bit digit at `shift`: (skeys, sidx) -> (w.keys[q], w.idx[q]); sidx == nullptr is the identity
hipError_t radix_pass(hipStream_t s, const Workspace &w, const int32_t *skeys, const int32_t *sidx, int64_t nnz, int shift, int q)
{
    radix_hist_kernel<<<(unsigned)w.tiles, T_THREADS, 0, s>>>(skeys, nnz, shift, w.tiles, w.hist);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = scan_exclusive(s, w.hist, w.hist_len, w.bsum, w.scan_blocks);
    if (e != hipSuccess) return e;
    radix_scatter_kernel<<<(unsigned)w.tiles, T_THREADS, 0, s>>>(skeys, sidx, nnz, shift, w.tiles, w.hist, w.keys[q], w.idx[q]);
    return hipGetLastError();
}

} // namespace
