// host_rt.h -- the host runtime pieces every file of the C ABI shares (api.hip, coalesce.hip, multi.hip,
// txpipe.hip): grow-only device and pinned buffers, the device scope, the HIP error message, and the
// stream drain that makes "an error return leaves nothing of the call running" a property of a type.
// Host-only C++17, no kernels (tools/hostrt_check.cpp builds it with a plain host compiler).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <string>
#include "../../include/bcos_gpu.h"

namespace bcosgpu {

// the growth rule of both buffers: the capacity after ensure(bytes) on a buffer of capacity `cap` -- kept
// while it suffices, else the floor `min` or the request plus a quarter of headroom
inline size_t grown_cap(size_t cap, size_t bytes, size_t min) {
    return bytes <= cap ? cap : bytes < min ? min : bytes + bytes / 4;
}

// Grow-only device buffer (contents are not kept across a growth; a failed ensure leaves it empty).
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    size_t min = 4096;
    hipError_t ensure(size_t bytes) {
        const size_t want = grown_cap(cap, bytes, min);
        if (want == cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        else p = nullptr;
        return e;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// Grow-only pinned host buffer; `mapped` maps it into the device's address space at hd (zero-copy).
struct PinnedBuf {
    void* p = nullptr;
    void* hd = nullptr;
    size_t cap = 0;
    bool mapped = false;
    explicit PinnedBuf(bool map = false) : mapped(map) {}
    hipError_t ensure(size_t bytes) {
        const size_t want = grown_cap(cap, bytes, 65536);
        if (want == cap) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = hd = nullptr;
        cap = 0;
        hipError_t e = hipHostMalloc(&p, want, mapped ? hipHostMallocMapped : hipHostMallocDefault);
        if (e != hipSuccess) p = nullptr;
        else if (mapped && (e = hipHostGetDevicePointer(&hd, p, 0)) != hipSuccess) {
            (void)hipHostFree(p);  // (unmapped it is of no use: leave the buffer empty, as after any failure)
            p = hd = nullptr;
        }
        if (e == hipSuccess) cap = want;
        return e;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// Selects `dev` on the calling thread for the scope (err: why it could not) and puts the old device back.
struct DeviceScope {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceScope(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) {
            (void)hipGetLastError();
            prev = -1;
        }
        if (prev != dev && (err = hipSetDevice(dev)) != hipSuccess) (void)hipGetLastError();  // (reported in err)
    }
    ~DeviceScope() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};

inline std::string hip_msg(hipError_t e, const char* what) { return std::string(what) + ": " + hipGetErrorString(e); }

// in a function with a `std::string& msg`: a failed HIP call leaves its message there and returns E_HIP
#define HIP_TRY(call)                     \
    do {                                  \
        const hipError_t e_ = (call);     \
        if (e_ != hipSuccess) {           \
            msg = hip_msg(e_, #call);     \
            return BCOSGPU_E_HIP;         \
        }                                 \
    } while (0)

// Declared before a call's first enqueue on its streams: every return that is not preceded by dismiss()
// first waits for the streams (results swallowed: the return already carries the first error), so an
// error return leaves no work of the call running on the GPU or writing the caller's memory.  dismiss()
// follows the synchronisation that ends the success path, which therefore gains no call.  A caller's
// `return f(hipGetLastError(), ...)` evaluates its message before this destructor runs.
class StreamDrain {
public:
    explicit StreamDrain(hipStream_t a, hipStream_t b = nullptr, hipStream_t c = nullptr) : s_{a, b, c} {}
    ~StreamDrain() {
        if (armed_)
            for (hipStream_t s : s_)
                if (s) (void)hipStreamSynchronize(s);
    }
    void dismiss() { armed_ = false; }
    StreamDrain(const StreamDrain&) = delete;
    StreamDrain& operator=(const StreamDrain&) = delete;

private:
    hipStream_t s_[3];
    bool armed_ = true;
};

}  // namespace bcosgpu
