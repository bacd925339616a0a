// capi_util.h -- helpers of the C-ABI entry points (capi.hip, transpose.hip, coo.hip, the structure plans): argument checks,
// the device switch of a call, the device buffers a plan owns, and a structure's way to the host and a plan's to the device.
// Internal to each translation unit: nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <utility>
#include <vector>
#include "../../include/sblas_hip.h"

namespace {

struct DeviceScope {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceScope(int dev)
    {
        if (dev < 0) return;
        err = hipGetDevice(&prev);
        if (err != hipSuccess) return;
        if (prev != dev) {
            err = hipSetDevice(dev);
            switched = (err == hipSuccess);
            if (!switched) (void)hipGetLastError(); // reported through err: the next launch check must not see it again
        }
    }
    ~DeviceScope()
    {
        if (switched) (void)hipSetDevice(prev);
    }
};

// the device a `dev` argument means (dev < 0: the calling thread's current device); -1 when that cannot be told
inline int resolve_device(int dev)
{
    if (dev >= 0) return dev;
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) return -1;
    return cur;
}

// dense operand layouts (SBLAS_COL_MAJOR / SBLAS_ROW_MAJOR)
inline bool order_ok(int order) { return order == SBLAS_COL_MAJOR || order == SBLAS_ROW_MAJOR; }
// leading dimension of a dense operand with `rows` rows and n columns: column-major needs ld >= rows, row-major ld >= n
inline bool ld_ok(int order, int64_t ld, int64_t rows, int64_t n) { return ld >= (order == SBLAS_ROW_MAJOR ? n : rows); }
// column j0 of a dense operand
template <typename T> inline T *col_at(T *p, int order, int64_t ld, int64_t j0) { return p + (order == SBLAS_ROW_MAJOR ? j0 : j0 * ld); }

inline bool csr_args_ok(int64_t rows, int64_t cols, int64_t nnz, const void *rowptr, const void *colidx,
                        const void *val)
{
    if (rows < 0 || cols < 0 || nnz < 0) return false;
    if (rows > INT_MAX - 64 || cols > INT_MAX || nnz > INT_MAX) return false; // int32 index API
    if (!rowptr) return false;
    if (nnz > 0 && (!colidx || !val)) return false;
    return true;
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; } // Bt: 16-byte tile loads
inline size_t pad256(size_t b) { return (b + 255) / 256 * 256; } // a segment of a solver plan's one buffer

// One device allocation of a plan.  It is made on the current device (the caller's DeviceScope) and freed on the device
// it was made for, whichever device is current then.
class DeviceBuffer {
public:
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    DeviceBuffer(DeviceBuffer &&o) noexcept : p_(o.p_), dev_(o.dev_) { o.p_ = nullptr; }
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept
    {
        std::swap(p_, o.p_), std::swap(dev_, o.dev_);
        return *this;
    }
    ~DeviceBuffer()
    {
        if (!p_) return;
        DeviceScope scope(dev_);
        (void)hipFree(p_);
    }
    hipError_t alloc(int dev, size_t bytes)
    {
        dev_ = dev;
        return hipMalloc(&p_, bytes);
    }
    // the buffer from byte `offset` on, as T
    template <typename T> T *at(size_t offset = 0) const { return reinterpret_cast<T *>(static_cast<char *>(p_) + offset); }
    explicit operator bool() const { return p_ != nullptr; }

private:
    void *p_ = nullptr;
    int dev_ = -1;
};

// (rowptr, colidx) of an n-row structure (n > 0) brought to the host once on stream s, which is synchronised: every check
// and the whole schedule of a structure plan are host work.  A rowptr that does not end at nnz is refused here, as row
// n - 1 and before every other check: the host rules follow rowptr into a colidx of nnz entries.
inline int fetch_structure(hipStream_t s, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx,
                           std::vector<int32_t> &h_rowptr, std::vector<int32_t> &h_colidx, int64_t *bad_row)
{
    h_rowptr.resize((size_t)n + 1), h_colidx.resize((size_t)nnz);
    hipError_t e = hipMemcpyAsync(h_rowptr.data(), rowptr, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && nnz > 0) e = hipMemcpyAsync(h_colidx.data(), colidx, (size_t)nnz * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return SBLAS_E_HIP;
    if (h_rowptr[n] != nnz) {
        if (bad_row) *bad_row = n - 1;
        return SBLAS_E_INVALID;
    }
    return SBLAS_OK;
}

// A host array on its way into a plan's buffer; offset: where upload_segments() put it.
struct Segment {
    const void *src;
    size_t bytes, offset;
    template <typename T> explicit Segment(const std::vector<T> &v) : src(v.data()), bytes(v.size() * sizeof(T)), offset(0) {}
};

// Allocates buf on dev for the segments one after another, each padded to 16 bytes, and uploads them on s, which is
// synchronised: the host arrays are read until here.  *total: the bytes allocated.
inline hipError_t upload_segments(DeviceBuffer &buf, int dev, hipStream_t s, Segment *seg, int count, size_t *total)
{
    *total = 0;
    for (int k = 0; k < count; ++k) seg[k].offset = *total, *total += (seg[k].bytes + 15) / 16 * 16;
    hipError_t e = buf.alloc(dev, *total);
    for (int k = 0; k < count && e == hipSuccess; ++k)
        e = hipMemcpyAsync(buf.at<char>(seg[k].offset), seg[k].src, seg[k].bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e;
}

} // namespace
