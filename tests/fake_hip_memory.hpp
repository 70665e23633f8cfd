// fake_hip_memory.hpp - TESTS ONLY: what tests/host_memory_driver.cpp, tests/call_memory_driver.cpp and tests/env_schedule_driver.cpp read of the stand-in in
// fake_hip_memory.cpp.
#pragma once
#include <cstddef>
#include <string>

namespace fake_hip {
struct Counters {
    int malloc_ = 0, free_ = 0, host_malloc = 0, host_free = 0, sync = 0;
    int copy = 0, copy2d = 0, attributes = 0, last_error = 0;
    int total() const { return malloc_ + free_ + host_malloc + host_free + sync + copy + copy2d + attributes + last_error; }
};
extern Counters counters;
extern std::string log;             // one letter per call, in order: M F (device), m f (pinned), S (synchronize),
                                    // U D (hipMemcpyAsync up / down), u d (hipMemcpy2DAsync up / down), A (pointer attributes), E (last error)
extern int fail_allocation_in;      // n > 0: the n-th allocation from now fails with hipErrorOutOfMemory
extern int fail_copy_in;            // n > 0: the n-th copy from now (of either kind) fails with hipErrorInvalidValue and moves nothing
extern size_t last_bytes;           // size of the last successful allocation
extern int bad_frees;               // frees of a block that was not live (or of the other kind)
size_t live();                      // blocks allocated and not freed
// what hipPointerGetAttributes reports of a pointer: device memory of `ordinal`, host memory (ordinal < 0), or - a pointer never
// marked - hipErrorInvalidValue, which stays the sticky error until hipGetLastError takes it
void mark(const void* p, int ordinal);
}  // namespace fake_hip
