// soc_devbuf.h -- the one type that owns device memory, for the host code of libsoc_hip.so: the handle (soc_host.h) and what its
// brick sweeps keep on the device (the host section of soc_brick.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>

#define SOC_HIDDEN __attribute__((visibility("hidden")))

// bytes of device memory that owning DevBufs hold, all handles of the process together (soc_device_bytes)
extern SOC_HIDDEN std::atomic<int64_t> soc_dev_bytes;

// n elements of device memory at p: the library's own (owned: freed by release() and by the destructor) or a caller's (bind)
template <typename T>
struct DevBuf {
    T     *p = nullptr;
    size_t n = 0;                      // capacity in elements (an owned buffer of 0 elements is allocated with one)
    bool   owned = false;

    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n), owned(o.owned) { o.p = nullptr;  o.n = 0;  o.owned = false; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { release();  p = o.p;  n = o.n;  owned = o.owned;  o.p = nullptr;  o.n = 0;  o.owned = false; }
        return *this;
    }
    ~DevBuf() { release(); }

    operator T *() const { return p; }
    explicit operator bool() const { return p != nullptr; }
    size_t bytes() const { return (n ? n : 1) * sizeof(T); }

    void release()
    {
        if (p && owned) { (void)hipFree(p);  soc_dev_bytes -= (int64_t)bytes(); }
        p = nullptr;  n = 0;  owned = false;
    }
    // a caller's memory: used, never freed
    void bind(T *ptr, size_t count) { release();  p = ptr;  n = count;  owned = false; }
    // exactly `need` elements of the library's own, whatever is held; the contents are not kept.  The stream drains before a buffer
    // goes (a launch in flight may still read it); a failed wait leaves it in place
    hipError_t reset(size_t need, hipStream_t stream)
    {
        if (p) { hipError_t e = hipStreamSynchronize(stream);  if (e != hipSuccess) return e; }
        release();
        hipError_t e = hipMalloc((void **)&p, (need ? need : 1) * sizeof(T));
        if (e != hipSuccess) { p = nullptr;  return e; }
        n = need;  owned = true;
        soc_dev_bytes += (int64_t)bytes();
        return hipSuccess;
    }
    // at least `need` elements: nothing to do when they are there, else reset(need)
    hipError_t reserve(size_t need, hipStream_t stream) { return n >= need ? hipSuccess : reset(need, stream); }
};
