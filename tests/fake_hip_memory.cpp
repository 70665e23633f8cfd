// fake_hip_memory.cpp - TESTS ONLY.  The five HIP entry points raptor_amd/csrc/rq_memory.hpp calls (hipMalloc, hipFree,
// hipHostMalloc, hipHostFree, hipStreamSynchronize) and the four more of raptor_amd/csrc/rq_call_memory.hpp (hipMemcpyAsync,
// hipMemcpy2DAsync, hipPointerGetAttributes, hipGetLastError) on the host: blocks come from malloc, copies really move bytes, every
// call is counted and logged in order, the n-th allocation or the n-th copy from now can be told to fail, and a pointer is device
// memory of the ordinal it was marked with.  Built by tests/test_host_memory.py with g++ under AddressSanitizer + UBSan, so a block
// freed twice or never, or a copy past a block's end, is the sanitizer's finding as well as this file's.
#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>

#include "fake_hip_memory.hpp"

namespace fake_hip {
Counters counters;
std::string log;
int fail_allocation_in = 0, fail_copy_in = 0;
std::map<const void*, int> marks;
hipError_t sticky = hipSuccess;
void mark(const void* p, int ordinal) { marks[p] = ordinal; }
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
static bool copy_fails(hipMemcpyKind kind, char up, char down) {
    log += kind == hipMemcpyHostToDevice ? up : down;
    return fail_copy_in > 0 && --fail_copy_in == 0;
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
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t) {
    ++counters.copy;
    if (copy_fails(kind, 'U', 'D')) return hipErrorInvalidValue;
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipMemcpy2DAsync(void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t width, size_t height,
                            hipMemcpyKind kind, hipStream_t) {
    ++counters.copy2d;
    if (copy_fails(kind, 'u', 'd')) return hipErrorInvalidValue;
    for (size_t r = 0; r < height; ++r)
        std::memcpy(static_cast<char*>(dst) + r * dst_pitch, static_cast<const char*>(src) + r * src_pitch, width);
    return hipSuccess;
}
hipError_t hipPointerGetAttributes(hipPointerAttribute_t* at, const void* p) {
    ++counters.attributes; log += 'A';
    const auto it = marks.find(p);
    if (it == marks.end()) return sticky = hipErrorInvalidValue;
    at->type = it->second < 0 ? hipMemoryTypeHost : hipMemoryTypeDevice;
    at->device = it->second < 0 ? 0 : it->second;
    return hipSuccess;
}
hipError_t hipGetLastError(void) { ++counters.last_error; log += 'E'; const hipError_t e = sticky; sticky = hipSuccess; return e; }
}
