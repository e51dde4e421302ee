// lfm_buffers.h -- the two grow-only buffer owners of the host engine: device
// memory and pinned host memory that a caller asks for by size before each
// use and that stay allocated between calls.
//
// Both have one rule: reserve(n) returns the buffer if it already holds n
// bytes, otherwise it frees the old allocation FIRST and then makes one of
// exactly n bytes (so the peak never holds both, and the contents are not
// preserved).  A buffer never shrinks.  reserve returns null on failure (the
// buffer is then empty); the HIP error is left for the caller to clear.
#pragma once
#include <cstddef>
#include <hip/hip_runtime.h>

#pragma GCC visibility push(hidden)
namespace lfm {

inline hipError_t device_alloc(void** p, size_t n) { return hipMalloc(p, n); }
inline hipError_t pinned_alloc(void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }

template <hipError_t (*ALLOC)(void**, size_t), hipError_t (*FREE)(void*)>
class GrowBuffer {
public:
    GrowBuffer() = default;
    GrowBuffer(const GrowBuffer&) = delete;
    GrowBuffer& operator=(const GrowBuffer&) = delete;
    // (movable: a caller may take a buffer out of a set that is released meanwhile)
    GrowBuffer& operator=(GrowBuffer&& o) noexcept
    {
        if (this != &o) {
            release();
            p_ = o.p_, cap_ = o.cap_;
            o.p_ = nullptr, o.cap_ = 0;
        }
        return *this;
    }
    GrowBuffer(GrowBuffer&& o) noexcept { *this = static_cast<GrowBuffer&&>(o); }
    ~GrowBuffer() { release(); }
    void* reserve(size_t n)
    {
        if (p_ && n <= cap_) return p_;
        release();
        if (ALLOC(&p_, n) != hipSuccess) {
            p_ = nullptr;
            return nullptr;
        }
        cap_ = n;
        return p_;
    }
    void release()
    {
        if (p_) (void)FREE(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    void* get() const { return p_; }

private:
    void* p_ = nullptr;
    size_t cap_ = 0;
};

using DeviceBuffer = GrowBuffer<device_alloc, hipFree>;      // hipMalloc
using HostBuffer = GrowBuffer<pinned_alloc, hipHostFree>;    // pinned host memory (hipHostMallocDefault)

} // namespace lfm
#pragma GCC visibility pop
