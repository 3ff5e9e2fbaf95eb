// device_buffer.h — owners of what the HIP runtime hands out: device memory, pinned host memory, events.  Move-only; the destructor gives back.
// Used by the context (hs_context.h) and by the load-time re-tiler (gpu_tiles.h).  Member functions that call the runtime are templates'
// members: a translation unit that gives `Free` itself and never allocates needs the HIP headers only (tests/cpp/test_device_buffer.cpp).
#ifndef HISPARSE_DEVICE_BUFFER_H_
#define HISPARSE_DEVICE_BUFFER_H_

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <utility>

template <typename T, hipError_t (*Free)(void*) = hipFree>
class DeviceBuffer {
public:
    DeviceBuffer() = default;
    ~DeviceBuffer() { reset(); }
    DeviceBuffer(DeviceBuffer&& o) noexcept : p_(o.release()) {}      // (declaring the moves deletes the copies)
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept { if (this != &o) adopt(o.release()); return *this; }
    hipError_t alloc(size_t bytes) { reset(); return hipMalloc(reinterpret_cast<void**>(&p_), bytes); }      // device memory (whatever was held is freed first)
    hipError_t alloc_count(size_t n, size_t min_bytes = 0) { return alloc(std::max(n * sizeof(T), min_bytes)); }      // n elements, at least min_bytes
    void adopt(T* raw) { if (p_) (void)Free(p_); p_ = raw; }
    T* release() { T* p = p_; p_ = nullptr; return p; }
    void reset() { adopt(nullptr); }
    T* get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }

private:
    T* p_ = nullptr;
};

template <typename T>
using PinnedBuffer = DeviceBuffer<T, hipHostFree>;      // hipHostMalloc'ed memory: adopt() the pointer

class DeviceEvent {
public:
    DeviceEvent() = default;
    ~DeviceEvent() { if (e_) (void)hipEventDestroy(e_); }
    DeviceEvent(DeviceEvent&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    DeviceEvent& operator=(DeviceEvent&& o) noexcept { std::swap(e_, o.e_); return *this; }      // (o's destructor gives the old one back)
    hipError_t create(unsigned flags = hipEventDefault) { return e_ ? hipSuccess : hipEventCreateWithFlags(&e_, flags); }
    hipEvent_t get() const { return e_; }

private:
    hipEvent_t e_ = nullptr;
};

#endif  // HISPARSE_DEVICE_BUFFER_H_
