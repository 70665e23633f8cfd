// rq_call_memory.hpp - the `memory` argument (RQ_DST_HOST / _DEVICE / _DEVICE_ASYNC) of the calls that read a recorded trajectory, as
// one object per call.  Host arrays go through staging memory the caller has reserved (in: copied up at once; out: copied back by
// finish, in the order they were named), device arrays are used where they lie, and finish() waits for the stream unless the call is
// only enqueued.  No allocation, nothing virtual: a mode, a stream, at most three copies owed.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>

#include "../../include/raptor_quad.h"

namespace rq {

class CallMemory {
public:
    static bool valid(int mode) { return mode >= RQ_DST_HOST && mode <= RQ_DST_DEVICE_ASYNC; }
    CallMemory(int mode, hipStream_t stream, int ordinal) : mode_(mode), ordinal_(ordinal), stream_(stream) {}
    bool host() const { return mode_ == RQ_DST_HOST; }

    // is p device memory of this call's device?  (a host-memory call has no such array: false, and nothing is asked)
    bool on_device(const void* p) const {
        if (host()) return false;
        hipPointerAttribute_t at{};
        const hipError_t e = hipPointerGetAttributes(&at, p);
        if (e != hipSuccess) (void)hipGetLastError();         // the query's own error must not meet the next launch
        return e == hipSuccess && at.type == hipMemoryTypeDevice && at.device == ordinal_;
    }
    // *dev: an input array as the launch takes it - a host array is copied into `stage` first
    template <typename T>
    hipError_t in(const T* src, size_t count, T* stage, const T** dev) const {
        *dev = host() ? stage : src;
        return host() ? hipMemcpyAsync(stage, src, count * sizeof(T), hipMemcpyHostToDevice, stream_) : hipSuccess;
    }
    // -> an output array as the launch takes it: `stage` for a host array, which finish() then fills from it.  The second form: `rows`
    // rows whose first `cols` columns are the call's - only those go back, the caller's columns cols .. ld_dst-1 stay as they were
    template <typename T> T* out(T* dst, size_t count, T* stage) { return static_cast<T*>(owe({dst, stage, count * sizeof(T), 0, 0, 0})); }
    template <typename T>
    T* out(T* dst, size_t ld_dst, T* stage, size_t ld_stage, size_t cols, size_t rows) {
        return static_cast<T*>(owe({dst, stage, cols * sizeof(T), ld_dst * sizeof(T), ld_stage * sizeof(T), rows}));
    }
    // the copies owed, then the wait (RQ_DST_DEVICE_ASYNC: neither).  The first failure is returned and nothing follows it.
    hipError_t finish() {
        if (owed_ > kMaxOwed) return hipErrorInvalidValue;
        for (int k = 0; k < owed_; ++k) {
            const Owed& c = copies_[k];
            const hipError_t e = c.rows ? hipMemcpy2DAsync(c.dst, c.dst_pitch, c.stage, c.stage_pitch, c.bytes, c.rows, hipMemcpyDeviceToHost, stream_)
                                        : hipMemcpyAsync(c.dst, c.stage, c.bytes, hipMemcpyDeviceToHost, stream_);
            if (e != hipSuccess) return e;
        }
        return mode_ == RQ_DST_DEVICE_ASYNC ? hipSuccess : hipStreamSynchronize(stream_);
    }

private:
    static constexpr int kMaxOwed = 3;           // no entry point names more (the backward: dL/dtheta and dL/dh_start)
    struct Owed { void* dst; void* stage; size_t bytes, dst_pitch, stage_pitch, rows; };      // rows == 0: one run of bytes
    void* owe(const Owed& c) {
        if (!host()) return c.dst;
        if (owed_ < kMaxOwed) copies_[owed_] = c;
        ++owed_;                                 // one too many: finish() refuses
        return c.stage;
    }
    int mode_, ordinal_, owed_ = 0;
    hipStream_t stream_;
    Owed copies_[kMaxOwed];
};

}  // namespace rq
