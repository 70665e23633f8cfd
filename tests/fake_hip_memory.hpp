// fake_hip_memory.hpp - TESTS ONLY: what tests/host_memory_driver.cpp reads of the stand-in in fake_hip_memory.cpp.
#pragma once
#include <cstddef>
#include <string>

namespace fake_hip {
struct Counters {
    int malloc_ = 0, free_ = 0, host_malloc = 0, host_free = 0, sync = 0;
    int total() const { return malloc_ + free_ + host_malloc + host_free + sync; }
};
extern Counters counters;
extern std::string log;             // one letter per call, in order: M F (device), m f (pinned), S (synchronize)
extern int fail_allocation_in;      // n > 0: the n-th allocation from now fails with hipErrorOutOfMemory
extern size_t last_bytes;           // size of the last successful allocation
extern int bad_frees;               // frees of a block that was not live (or of the other kind)
size_t live();                      // blocks allocated and not freed
}  // namespace fake_hip
