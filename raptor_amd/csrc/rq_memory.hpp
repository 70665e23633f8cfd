// rq_memory.hpp - the one owner of device and pinned host memory in the host layer of libraptor_quad.so.  Every object behind a handle
// holds its blocks through these two types: a block is freed when its owner goes (`delete` inside the entry point's DeviceScope), a
// half-built object needs no unwinding, and "grow this scratch buffer" is reserve() - one rule for every site.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>

namespace rq {

template <typename T, bool kPinned>
class Buffer {
public:
    Buffer() = default;
    Buffer(Buffer&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    Buffer& operator=(Buffer&& o) noexcept { if (this != &o) { reset(); swap(o); } return *this; }
    Buffer(const Buffer&) = delete;
    Buffer& operator=(const Buffer&) = delete;
    ~Buffer() { reset(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t count() const { return n_; }          // elements it can hold
    bool empty() const { return p_ == nullptr; }

    // for an empty buffer; on failure it stays empty
    hipError_t alloc(size_t count) {
        void* p = nullptr;
        const hipError_t e = kPinned ? hipHostMalloc(&p, count * sizeof(T), hipHostMallocDefault) : hipMalloc(&p, count * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(p); n_ = count;
        return hipSuccess;
    }

    // Room for `count` elements.  Enough already: nothing happens, no HIP call.  Otherwise a block of max(count, floor) replaces the
    // one held - contents are not kept - after `stream` has drained: a launch may still read the old block.  A failed allocation
    // leaves the buffer empty (a failed synchronize: as it was).
    hipError_t reserve(hipStream_t stream, size_t count, size_t floor = 0) {
        if (n_ >= count) return hipSuccess;
        if (p_) {
            const hipError_t e = hipStreamSynchronize(stream);
            if (e != hipSuccess) return e;
            reset();
        }
        return alloc(count < floor ? floor : count);
    }

    // take over a block that hipFree releases and another HIP allocator made (fine-grained device memory)
    void adopt(T* p, size_t count) { reset(); p_ = p; n_ = count; }

    void reset() {
        if (p_) (void)(kPinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr; n_ = 0;
    }
    void swap(Buffer& o) noexcept { T* p = p_; p_ = o.p_; o.p_ = p; const size_t n = n_; n_ = o.n_; o.n_ = n; }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

template <typename T> using DeviceBuffer = Buffer<T, false>;
template <typename T> using PinnedBuffer = Buffer<T, true>;

}  // namespace rq
