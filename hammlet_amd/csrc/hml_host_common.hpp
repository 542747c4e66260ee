// Shared by the translation units of libhammlet_hip.so: the thread's last error message and the HIP call checks.
#ifndef HML_HOST_COMMON_HPP
#define HML_HOST_COMMON_HPP

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <string>
#include <utility>

#include "../../include/hml.h"

// stores the message hml_last_error() returns (hml_capi.hip) and passes the code through
int hml_set_err(int code, const std::string& msg);

#define HIPCHK(call)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return hml_set_err(HML_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));       \
    } while (0)

#define KLAUNCH_CHECK() HIPCHK(hipGetLastError())

// The one owner of device memory of the chain code, the text reader and the pooling code: a buffer is freed when its owner
// goes (a context's member with the context, scratch on every path out of a function - HIPCHK returns early), and nothing else
// calls hipMalloc / hipFree.  What the owners hold is counted (hml_device_memory_live), and a test can make the n-th allocation
// from now fail (hml_debug_fail_allocation): the failure paths are otherwise unreachable.
inline std::atomic<uint64_t> hml_dev_live_bytes{0}, hml_dev_live_allocations{0};
inline std::atomic<int64_t> hml_dev_alloc_seen{0}, hml_dev_alloc_fail_at{0};   // allocations since the hook was armed; the one that fails (0: none)

// Test mode (hml_debug_guard_allocations): while hml_dev_guard_bytes is not 0 an allocation is
// guard + bytes + guard, both guards hold a pattern, the body is 0xFF with hml_dev_guard_poison, and the allocation is
// registered until it is freed.  hml_guard.hip has the registry; with the mode off neither function is called.
inline std::atomic<uint64_t> hml_dev_guard_bytes{0};
inline std::atomic<int> hml_dev_guard_poison{0};
hipError_t hml_guard_alloc(void** user, uint64_t bytes, uint64_t guard, bool poison, int64_t ordinal);   // *user: the body
void hml_guard_free(void* user);   // waits for the device, checks both guards (into the sticky report), frees the whole

class DevBuf {
    void* p_ = nullptr;
    uint64_t bytes_ = 0;
    bool guarded_ = false;
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { free(); }
    // frees what it held, then allocates anew (a failure leaves it empty)
    hipError_t alloc(uint64_t bytes) {
        free();
        const int64_t ordinal = ++hml_dev_alloc_seen;
        if (ordinal == hml_dev_alloc_fail_at.load()) { hml_dev_alloc_fail_at = 0; return hipErrorOutOfMemory; }
        const uint64_t guard = hml_dev_guard_bytes.load();
        const bool guarded = guard != 0 && bytes != 0;   // (a zero-byte request stays empty)
        const hipError_t e = guarded ? hml_guard_alloc(&p_, bytes, guard, hml_dev_guard_poison.load() != 0, ordinal) : hipMalloc(&p_, bytes);
        if (e != hipSuccess) { p_ = nullptr; return e; }
        if (p_) { bytes_ = bytes; guarded_ = guarded; hml_dev_live_bytes += bytes; hml_dev_live_allocations++; }
        return hipSuccess;
    }
    void free() {
        if (!p_) return;
        if (guarded_) hml_guard_free(p_); else (void)hipFree(p_);
        hml_dev_live_bytes -= bytes_; hml_dev_live_allocations--;
        p_ = nullptr; bytes_ = 0; guarded_ = false;
    }
    void swap(DevBuf& o) { std::swap(p_, o.p_); std::swap(bytes_, o.bytes_); std::swap(guarded_, o.guarded_); }   // (both stay counted: nothing is allocated or freed)
    explicit operator bool() const { return p_ != nullptr; }
    void* get() const { return p_; }
    template <class T> T* as() const { return static_cast<T*>(p_); }
};

// ... of n elements of T: reads as the T* it holds
template <class T> struct DevArr : DevBuf {
    hipError_t alloc(uint64_t n) { return DevBuf::alloc(n * sizeof(T)); }
    T* get() const { return as<T>(); }
    operator T*() const { return get(); }
    T* operator->() const { return get(); }
};

#endif
