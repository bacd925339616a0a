// capi_util.h -- helpers of the C-ABI entry points (capi.hip, transpose.hip, coo.hip): argument checks, the device switch of a
// call and the device buffers a plan owns.  Internal to each translation unit: nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <utility>
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

} // namespace
