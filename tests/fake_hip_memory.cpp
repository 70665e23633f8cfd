// fake_hip_memory.cpp - TESTS ONLY.  The five HIP entry points raptor_amd/csrc/rq_memory.hpp calls (hipMalloc, hipFree,
// hipHostMalloc, hipHostFree, hipStreamSynchronize) on the host: blocks come from malloc, every call is counted and logged in
// order, and the n-th allocation from now can be told to fail.  Built by tests/test_host_memory.py with g++ under
// AddressSanitizer + UBSan, so a block freed twice or never is the sanitizer's finding as well as this file's.
#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <set>
#include <string>

#include "fake_hip_memory.hpp"

namespace fake_hip {
Counters counters;
std::string log;
int fail_allocation_in = 0;
std::set<void*> device_blocks, pinned_blocks;
size_t last_bytes = 0;
int bad_frees = 0;

static hipError_t allocate(void** p, size_t bytes, std::set<void*>& blocks, char tag) {
    log += tag;
    if (fail_allocation_in > 0 && --fail_allocation_in == 0) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = std::malloc(bytes ? bytes : 1);
    blocks.insert(*p);
    last_bytes = bytes;
    return hipSuccess;
}
static hipError_t release(void* p, std::set<void*>& blocks, char tag) {
    log += tag;
    if (blocks.erase(p) != 1) { ++bad_frees; return hipErrorInvalidValue; }      // not live, or of the other kind
    std::free(p);
    return hipSuccess;
}
size_t live() { return device_blocks.size() + pinned_blocks.size(); }
}  // namespace fake_hip

using namespace fake_hip;

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { ++counters.malloc_; return allocate(p, bytes, device_blocks, 'M'); }
hipError_t hipFree(void* p) { ++counters.free_; return release(p, device_blocks, 'F'); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { ++counters.host_malloc; return allocate(p, bytes, pinned_blocks, 'm'); }
hipError_t hipHostFree(void* p) { ++counters.host_free; return release(p, pinned_blocks, 'f'); }
hipError_t hipStreamSynchronize(hipStream_t) { ++counters.sync; log += 'S'; return hipSuccess; }
}
