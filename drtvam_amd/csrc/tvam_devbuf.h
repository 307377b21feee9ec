// tvam_devbuf.h — the one owner of device memory: every device allocation of the library is a
// TvamDevBuf, freed by its destructor and counted in tvam_device_bytes() (include/tvam.h).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <vector>

inline std::atomic<int64_t> g_tvam_device_bytes{0};  // device bytes the library owns in this process

template <typename T>
class TvamDevBuf {
public:
    TvamDevBuf() = default;
    TvamDevBuf(const TvamDevBuf&) = delete;
    TvamDevBuf& operator=(const TvamDevBuf&) = delete;
    TvamDevBuf(TvamDevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
    TvamDevBuf& operator=(TvamDevBuf&& o) noexcept {
        if (this != &o) {
            (void)reset();
            std::swap(p_, o.p_);
            std::swap(n_, o.n_);
        }
        return *this;
    }
    ~TvamDevBuf() { (void)reset(); }

    // n elements, uninitialised; whatever was held is freed first.  Holds nothing after a failure.
    hipError_t alloc(size_t n) {
        (void)reset();
        const hipError_t e = hipMalloc((void**)&p_, n * sizeof(T));
        if (e != hipSuccess) {
            p_ = nullptr;
            return e;
        }
        n_ = n;
        g_tvam_device_bytes += (int64_t)(n * sizeof(T));
        return hipSuccess;
    }
    // at least n elements; the contents do not survive a reallocation
    hipError_t grow(size_t n) { return n <= n_ ? hipSuccess : alloc(n); }
    // a copy of v (at least one element is allocated, so that get() is a valid pointer)
    hipError_t upload(const std::vector<T>& v) {
        hipError_t e = alloc(std::max<size_t>(v.size(), 1));
        if (e == hipSuccess && !v.empty()) e = hipMemcpy(p_, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
        return e;
    }
    hipError_t reset() {
        const hipError_t e = p_ ? hipFree(p_) : hipSuccess;
        g_tvam_device_bytes -= (int64_t)(n_ * sizeof(T));
        p_ = nullptr;
        n_ = 0;
        return e;
    }
    T* get() const { return p_; }
    size_t capacity() const { return n_; }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};
