// Owners of the engine's device and pinned host memory: the only place that calls the runtime's allocators (the
// trace passes' buffer list, capi_samples.hpp, aside).  A handle's buffers are DevArray members and free themselves
// with it; a C-ABI call's buffers are DevArray locals and free themselves when it returns.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

struct dlsm_chain;

namespace dlsm {

// files a failed runtime call on the handle the way HIPCHK does and returns DLSM_E_HIP (capi.hip)
int mem_fail(dlsm_chain *h, hipError_t e, const char *call);

// One hipMalloc'd array.  Converts to T * - kernel launches and ChainView take raw pointers - and is move-only.
template <typename T>
class DevArray {
    T *p_ = nullptr;
    size_t n_ = 0;

public:
    DevArray() = default;
    DevArray(DevArray &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DevArray &operator=(DevArray &&o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    ~DevArray() { reset(); }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    T *operator->() const { return p_; }            // the address of a device struct's member, never a host access
    size_t size() const { return n_; }              // elements asked for: the capacity of a grow-only buffer
    void reset() { if (p_) hipFree(p_); p_ = nullptr; n_ = 0; }
    // free, then allocate n elements (never a zero-byte request: n = 0 still leaves a valid pointer)
    int alloc(dlsm_chain *h, size_t n) {
        reset();
        hipError_t e = hipMalloc((void **)&p_, (n > 0 ? n : 1) * sizeof(T));
        if (e != hipSuccess) { p_ = nullptr; return mem_fail(h, e, "hipMalloc"); }
        n_ = n;
        return 0;
    }
    // grow-only: *moved tells the caller that the pointer changed (whoever holds the old one must let go of it)
    int ensure(dlsm_chain *h, size_t n, bool *moved = nullptr) {
        if (moved) *moved = n_ < n;
        return n_ < n ? alloc(h, n) : 0;
    }
};

// One hipHostMalloc'd array; of a mapped one, dev() is the address the device stores to.
enum : unsigned { HOST_PINNED = hipHostMallocDefault, HOST_MAPPED = hipHostMallocMapped,
                  HOST_MAPPED_PORTABLE = hipHostMallocMapped | hipHostMallocPortable };
template <typename T>
class HostArray {
    T *p_ = nullptr, *dev_ = nullptr;

public:
    HostArray() = default;
    HostArray(HostArray &&) = delete;
    ~HostArray() { if (p_) hipHostFree(p_); }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    T *dev() const { return dev_; }
    // (the callers differ in what a failure means - the staging buffer is optional - so the runtime's code comes back)
    hipError_t alloc(size_t n, unsigned flags = HOST_PINNED) {
        if (p_) hipHostFree(p_);
        dev_ = nullptr;
        hipError_t e = hipHostMalloc((void **)&p_, n * sizeof(T), flags);
        if (e != hipSuccess) { p_ = nullptr; return e; }
        if ((flags & hipHostMallocMapped) && hipHostGetDevicePointer((void **)&dev_, p_, 0) != hipSuccess) dev_ = nullptr;
        return hipSuccess;
    }
    T *release() { T *p = p_; p_ = dev_ = nullptr; return p; }     // to a pointer that lives as long as the process
};

}  // namespace dlsm
