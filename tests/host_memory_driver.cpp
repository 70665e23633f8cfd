// host_memory_driver.cpp - TESTS ONLY: rq::DeviceBuffer / rq::PinnedBuffer (raptor_amd/csrc/rq_memory.hpp) against the counting
// stand-in of fake_hip_memory.cpp.  Prints "ok" and returns 0, or names the first check that failed.
#include <cstdio>
#include <utility>

#include "../raptor_amd/csrc/rq_memory.hpp"
#include "fake_hip_memory.hpp"

using fake_hip::counters;

#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) { std::printf("FAILED line %d: %s (calls so far: %s)\n", __LINE__, #cond, fake_hip::log.c_str()); return 1; } \
    } while (0)

template <typename Buf>
static int exercise(const char* first_log, const char* grow_log) {
    hipStream_t stream = nullptr;
    {
        Buf a;
        CHECK(a.empty() && a.get() == nullptr && a.count() == 0);
        // growing an empty buffer does not synchronise
        fake_hip::log.clear();
        CHECK(a.reserve(stream, 100) == hipSuccess);
        CHECK(fake_hip::log == first_log && counters.sync == 0);
        CHECK(!a.empty() && a.count() == 100 && fake_hip::last_bytes == 100 * sizeof(float));
        float* const first = a.get();
        CHECK(static_cast<float*>(a) == first);
        first[99] = 1.0f;                                 // the block really holds count() elements (AddressSanitizer watches)
        // enough room: no call at all
        const int before = counters.total();
        CHECK(a.reserve(stream, 100) == hipSuccess && a.reserve(stream, 1) == hipSuccess && a.reserve(stream, 0, 1000) == hipSuccess);
        CHECK(counters.total() == before && a.get() == first && a.count() == 100);
        // growing a buffer that holds memory: synchronise, then free, then allocate
        fake_hip::log.clear();
        CHECK(a.reserve(stream, 101) == hipSuccess);
        CHECK(fake_hip::log == grow_log && counters.sync == 1);
        CHECK(a.count() == 101);
        // the floor is honoured, and is what count() reports
        CHECK(a.reserve(stream, 200, 4096) == hipSuccess);
        CHECK(a.count() == 4096 && fake_hip::last_bytes == 4096 * sizeof(float));
        CHECK(a.reserve(stream, 5000, 4096) == hipSuccess && a.count() == 5000);
        // a failed reserve leaves it empty, and empty it frees nothing later
        fake_hip::fail_allocation_in = 1;
        CHECK(a.reserve(stream, 6000) == hipErrorOutOfMemory);
        CHECK(a.get() == nullptr && a.count() == 0 && a.empty());
        // alloc: for an empty buffer; on failure it stays empty
        Buf b;
        fake_hip::fail_allocation_in = 1;
        CHECK(b.alloc(8) == hipErrorOutOfMemory && b.get() == nullptr && b.count() == 0);
        CHECK(b.alloc(8) == hipSuccess && b.count() == 8);
        CHECK(a.alloc(3) == hipSuccess);
        // swap exchanges pointer and count
        float* const pa = a.get(); float* const pb = b.get();
        const int calls = counters.total();
        a.swap(b);
        CHECK(a.get() == pb && a.count() == 8 && b.get() == pa && b.count() == 3 && counters.total() == calls);
        // a moved-from object is empty; moving makes no call
        Buf c(std::move(a));
        CHECK(a.empty() && a.count() == 0 && c.get() == pb && c.count() == 8 && counters.total() == calls);
        Buf d;
        CHECK(d.alloc(5) == hipSuccess);
        d = std::move(c);                                 // d's own block is freed, c's taken over
        CHECK(c.empty() && c.count() == 0 && d.get() == pb && d.count() == 8 && fake_hip::live() == 2);
        d.reset();
        CHECK(d.empty() && d.count() == 0 && fake_hip::live() == 1);
        d.reset();                                        // twice: nothing to free
    }
    // every allocation was freed exactly once when the owners went out of scope
    CHECK(fake_hip::live() == 0 && fake_hip::bad_frees == 0);
    return 0;
}

int main() {
    if (exercise<rq::DeviceBuffer<float>>("M", "SFM")) return 1;
    CHECK(counters.host_malloc == 0 && counters.host_free == 0);           // the device type never touches pinned memory
    const int device_allocs = counters.malloc_, device_frees = counters.free_;
    CHECK(device_frees == device_allocs - 2);                              // all but the two allocations that were made to fail
    counters = fake_hip::Counters{};
    if (exercise<rq::PinnedBuffer<float>>("m", "Sfm")) return 1;
    CHECK(counters.malloc_ == 0 && counters.free_ == 0);
    CHECK(counters.host_free == counters.host_malloc - 2);
    {   // adopt: a block another allocator made is released like the type's own
        void* p = nullptr;
        CHECK(hipMalloc(&p, 64) == hipSuccess);
        rq::DeviceBuffer<unsigned> e;
        e.adopt(static_cast<unsigned*>(p), 16);
        CHECK(e.get() == p && e.count() == 16);
    }
    CHECK(fake_hip::live() == 0 && fake_hip::bad_frees == 0);
    std::printf("ok\n");
    return 0;
}
