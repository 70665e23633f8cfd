// call_memory_driver.cpp - TESTS ONLY: rq::CallMemory (raptor_amd/csrc/rq_call_memory.hpp) against the counting stand-in of
// fake_hip_memory.cpp.  Prints "ok" and returns 0, or names the first check that failed.
#include <cstdio>
#include <cstring>

#include "../raptor_amd/csrc/rq_call_memory.hpp"
#include "../raptor_amd/csrc/rq_memory.hpp"
#include "fake_hip_memory.hpp"

using fake_hip::counters;
using rq::CallMemory;

#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) { std::printf("FAILED line %d: %s (calls so far: %s)\n", __LINE__, #cond, fake_hip::log.c_str()); return 1; } \
    } while (0)

constexpr int kOrdinal = 3;
constexpr size_t kRows = 5, kCols = 6, kLd = 9;          // the 2-D output: kCols of the caller's kLd columns, packed on the device
constexpr float kSentinel = -77.0f;

// one call in `mode`: an input, two outputs (the second 2-D), as an entry point makes it; the "launch" doubles the input into the
// first output and numbers the second.  `fail_copy`: which copy from the call's start fails (0: none).
static int one_call(int mode, int fail_copy) {
    hipStream_t stream = nullptr;
    rq::DeviceBuffer<float> stage_in, stage_out, stage_2d, dev_in, dev_out, dev_2d;
    CHECK(stage_in.alloc(4) == hipSuccess && stage_out.alloc(4) == hipSuccess && stage_2d.alloc(kRows * kCols) == hipSuccess);
    CHECK(dev_in.alloc(4) == hipSuccess && dev_out.alloc(4) == hipSuccess && dev_2d.alloc(kRows * kLd) == hipSuccess);
    float host_in[4] = {1.0f, 2.0f, 3.0f, 4.0f}, host_out[4] = {0.0f, 0.0f, 0.0f, 0.0f}, host_2d[kRows * kLd];
    for (float& v : host_2d) v = kSentinel;
    const bool host = mode == RQ_DST_HOST;
    std::memcpy(dev_in.get(), host_in, sizeof(host_in));
    const float* src = host ? host_in : dev_in.get();
    float* dst = host ? host_out : dev_out.get();
    float* dst_2d = host ? host_2d : dev_2d.get();

    fake_hip::log.clear();
    fake_hip::fail_copy_in = fail_copy;
    CallMemory mem(mode, stream, kOrdinal);
    CHECK(mem.host() == host);
    const float* d_in = nullptr;
    const hipError_t e_in = mem.in(src, 4, stage_in.get(), &d_in);
    if (host && fail_copy == 1) {          // a failed upload is the caller's to return: nothing else was asked of HIP
        CHECK(e_in == hipErrorInvalidValue && fake_hip::log == "U");
        return 0;
    }
    CHECK(e_in == hipSuccess && d_in == (host ? stage_in.get() : src));
    CHECK(fake_hip::log == (host ? "U" : ""));
    if (host) CHECK(std::memcmp(stage_in.get(), host_in, sizeof(host_in)) == 0);           // the input is staged
    float* d_out = mem.out(dst, 4, stage_out.get());
    float* d_2d = mem.out(dst_2d, kLd, stage_2d.get(), kCols, kCols, kRows);
    CHECK(d_out == (host ? stage_out.get() : dst) && d_2d == (host ? stage_2d.get() : dst_2d));
    CHECK(fake_hip::log == (host ? "U" : ""));                                             // naming an output asks nothing of HIP
    const size_t ld_2d = host ? kCols : kLd;
    for (int i = 0; i < 4; ++i) d_out[i] = 2.0f * d_in[i];
    for (size_t r = 0; r < kRows; ++r)
        for (size_t c = 0; c < kCols; ++c) d_2d[r * ld_2d + c] = (float)(r * 100 + c);

    const hipError_t e = mem.finish();
    if (host && fail_copy == 2) {          // the first owed copy fails: no later copy, no synchronise
        CHECK(e == hipErrorInvalidValue && fake_hip::log == "UD" && counters.sync == 0);
        CHECK(host_out[0] == 0.0f && host_2d[0] == kSentinel);
        return 0;
    }
    if (host && fail_copy == 3) {          // the second: the first has arrived, still no synchronise
        CHECK(e == hipErrorInvalidValue && fake_hip::log == "UDd" && counters.sync == 0);
        CHECK(host_out[3] == 8.0f && host_2d[0] == kSentinel);
        return 0;
    }
    CHECK(e == hipSuccess);
    // per mode, the exact log: one H2D per in, one D2H per out in the order they were named, one synchronise; a synchronise alone;
    // not one call
    CHECK(fake_hip::log == (host ? "UDdS" : mode == RQ_DST_DEVICE ? "S" : ""));
    if (host) {
        for (int i = 0; i < 4; ++i) CHECK(host_out[i] == 2.0f * host_in[i]);               // an output comes back
        for (size_t r = 0; r < kRows; ++r)
            for (size_t c = 0; c < kLd; ++c)       // the first kCols columns of every row arrive, the caller's other columns stay
                CHECK(host_2d[r * kLd + c] == (c < kCols ? (float)(r * 100 + c) : kSentinel));
    }
    return 0;
}

int main() {
    for (int mode = -1; mode <= 3; ++mode) CHECK(CallMemory::valid(mode) == (mode >= 0 && mode <= 2));

    for (int mode : {RQ_DST_HOST, RQ_DST_DEVICE, RQ_DST_DEVICE_ASYNC}) {
        counters = fake_hip::Counters{};
        if (one_call(mode, 0)) return 1;
        CHECK(counters.sync == (mode == RQ_DST_DEVICE_ASYNC ? 0 : 1));
        CHECK(counters.copy == (mode == RQ_DST_HOST ? 2 : 0) && counters.copy2d == (mode == RQ_DST_HOST ? 1 : 0));
        CHECK(counters.attributes == 0 && counters.last_error == 0);
    }
    for (int fail_copy = 1; fail_copy <= 3; ++fail_copy) {
        counters = fake_hip::Counters{};
        if (one_call(RQ_DST_HOST, fail_copy)) return 1;
        CHECK(fake_hip::fail_copy_in == 0);
    }
    {   // a fourth output is one too many: finish() refuses before it copies anything
        float a[1] = {0.0f}, stage[1] = {0.0f};
        CallMemory mem(RQ_DST_HOST, nullptr, kOrdinal);
        for (int k = 0; k < 4; ++k) CHECK(mem.out(a, 1, stage) == stage);
        fake_hip::log.clear();
        CHECK(mem.finish() == hipErrorInvalidValue && fake_hip::log.empty());
    }
    {   // on_device: device memory of this call's ordinal, and nothing else
        int here = 0, elsewhere = 0, on_host = 0, unknown = 0;
        fake_hip::mark(&here, kOrdinal);
        fake_hip::mark(&elsewhere, kOrdinal + 1);
        fake_hip::mark(&on_host, -1);
        for (int mode : {RQ_DST_DEVICE, RQ_DST_DEVICE_ASYNC}) {
            const CallMemory mem(mode, nullptr, kOrdinal);
            counters = fake_hip::Counters{};
            fake_hip::log.clear();
            CHECK(mem.on_device(&here) && !mem.on_device(&on_host) && !mem.on_device(&elsewhere));
            CHECK(fake_hip::log == "AAA" && counters.last_error == 0);
            CHECK(!mem.on_device(&unknown));                   // the query fails: false, and its sticky error is taken
            CHECK(fake_hip::log == "AAAAE" && counters.last_error == 1);
            CHECK(hipGetLastError() == hipSuccess);
        }
        const CallMemory mem(RQ_DST_HOST, nullptr, kOrdinal);  // a host-memory call asks nothing
        const int before = counters.total();
        CHECK(!mem.on_device(&here) && !mem.on_device(&on_host) && counters.total() == before);
    }
    CHECK(fake_hip::live() == 0 && fake_hip::bad_frees == 0);
    std::printf("ok\n");
    return 0;
}
