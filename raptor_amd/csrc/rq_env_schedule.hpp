// rq_env_schedule.hpp - the device-facing part of a schedule slot of an env (rq_env_set_wrench_schedule and its kin): which bank is
// attached, with which ids, the [ld] first rows (id * rows) every stepping kernel reads, and the number that names the attachment.
// One type for every kind of schedule; what a row means is the kernels' business.  Needs rq_memory.hpp and the HIP runtime API only
// (tests/env_schedule_driver.cpp holds it on the CPU); like rq::CallMemory it words no message: the entry points do.
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstdint>
#include <new>
#include <vector>

#include "rq_memory.hpp"

namespace rq {

// what went wrong, for the caller to word: `hip` is the failed call's error (copy, synchronize, zero)
struct FirstRowsStatus {
    enum What { ok, host_allocation, device_allocation, copy, synchronize, zero } what = ok;
    hipError_t hip = hipSuccess;
    explicit operator bool() const { return what != ok; }      // true: failed
};

// One id per env -> the [ld] first rows (id * rows; null ids: table 0; 0 behind the n envs) at dst on the device, synchronised before
// the pageable rows go away.  A schedule's rows and a reference bank's.
inline FirstRowsStatus upload_first_rows(hipStream_t stream, const uint32_t* ids, uint32_t n, uint32_t ld, uint32_t rows, uint32_t* dst) {
    std::vector<uint32_t> first;
    try {                                   // nothing throws across the boundary
        first.assign(ld, 0u);
    } catch (const std::bad_alloc&) {
        return {FirstRowsStatus::host_allocation};
    }
    for (uint32_t i = 0; ids && i < n; ++i) first[i] = ids[i] * rows;       // < n_tables * rows < 2^28
    hipError_t e = hipMemcpyAsync(dst, first.data(), (size_t)ld * sizeof(uint32_t), hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return {FirstRowsStatus::copy, e};
    e = hipStreamSynchronize(stream);                // `first` is pageable and goes away
    if (e != hipSuccess) return {FirstRowsStatus::synchronize, e};
    return {};
}

inline uint64_t fresh_attachment() {        // never 0, never twice
    static std::atomic<uint64_t> counter{0};
    return counter.fetch_add(1, std::memory_order_relaxed) + 1;
}

// Bank: anything with `rows` (of one table) and `attached` (live envs it is attached to: its destruction is refused while any).  A
// bank cannot be destroyed while it is attached, so the pointer is followed.
template <typename Bank>
struct EnvSchedule {
    Bank* bank = nullptr;
    std::vector<uint32_t> ids;          // one table per env, as attached (empty: none attached)
    DeviceBuffer<uint32_t> row0;        // [ld], reserved at the first attachment and kept
    uint64_t gen = 0;                   // names the attachment (0: none): a chained rollout's hipGraph is keyed by it

    EnvSchedule() = default;
    EnvSchedule(const EnvSchedule&) = delete;
    EnvSchedule& operator=(const EnvSchedule&) = delete;
    ~EnvSchedule() { detach(); }        // an env that goes lets its banks go

    // `to` with one id per env (null: table 0 for all) in place of what was attached.  The caller has drained the stream: a launch in
    // flight reads the first rows of the schedule before.  On failure the slot and both banks are as they were.
    FirstRowsStatus attach(hipStream_t stream, Bank* to, const uint32_t* id, uint32_t n, uint32_t ld) {
        std::vector<uint32_t> next;
        try {                               // nothing throws across the boundary
            if (id) next.assign(id, id + n); else next.assign(n, 0u);
        } catch (const std::bad_alloc&) {
            return {FirstRowsStatus::host_allocation};
        }
        if (row0.empty() && row0.alloc(ld) != hipSuccess) return {FirstRowsStatus::device_allocation};
        const FirstRowsStatus s = upload_first_rows(stream, id, n, ld, to->rows, row0);
        if (s) return s;
        if (bank) bank->attached -= 1;
        to->attached += 1;
        bank = to;
        ids.swap(next);
        gen = fresh_attachment();
        return {};
    }

    void detach() {
        if (bank) bank->attached -= 1;
        bank = nullptr; gen = 0; ids.clear();
    }
};

// The command history of an env's delay schedule (rq_env_set_delay_schedule): `floats` floats on the device, allocated at the first
// attachment and kept, zeroed at every attachment - commands from before an attachment read as zero.  attach() is the slot's, with
// the history made ready first: a failure anywhere leaves the slot and both banks as they were (a copy that fails behind the
// zeroing leaves the history zeroed and the schedule before attached: its commands of before read as zero).
struct DelayHistory {
    DeviceBuffer<float> ring;

    template <typename Bank>
    FirstRowsStatus attach(hipStream_t stream, EnvSchedule<Bank>& slot, Bank* to, const uint32_t* id, uint32_t n, uint32_t ld, size_t floats) {
        if (ring.empty() && ring.alloc(floats) != hipSuccess) return {FirstRowsStatus::device_allocation};
        // (stream-ordered: the caller has drained the stream, and every launch that reads the ring comes after)
        const hipError_t e = hipMemsetAsync(ring, 0, floats * sizeof(float), stream);
        if (e != hipSuccess) return {FirstRowsStatus::zero, e};
        return slot.attach(stream, to, id, n, ld);
    }
};

}  // namespace rq
