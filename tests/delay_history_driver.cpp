// delay_history_driver.cpp - TESTS ONLY: rq::DelayHistory (raptor_amd/csrc/rq_env_schedule.hpp), the command history an env keeps for
// its delay schedule, against the counting stand-in of fake_hip_memory.cpp.  Prints "ok" and returns 0, or names the first check that
// failed.
#include <cstdio>
#include <cstring>

#include "../raptor_amd/csrc/rq_env_schedule.hpp"
#include "fake_hip_memory.hpp"

// the one call of the history the stand-in does not have: counted here ('Z' in the log), it can be made to fail once
static int memsets = 0;
static bool fail_next_memset = false;
extern "C" hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t) {
    ++memsets;
    fake_hip::log += 'Z';
    if (fail_next_memset) { fail_next_memset = false; return hipErrorInvalidValue; }
    std::memset(dst, value, bytes);
    return hipSuccess;
}

using rq::FirstRowsStatus;

#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) { std::printf("FAILED line %d: %s (calls so far: %s)\n", __LINE__, #cond, fake_hip::log.c_str()); return 1; } \
    } while (0)

struct Bank { uint32_t rows = 0, attached = 0; };
using Slot = rq::EnvSchedule<Bank>;

constexpr uint32_t kN = 5, kLd = 64;
constexpr size_t kFloats = 32 * 4 * kLd;      // slots x action fields x ld

static bool all_zero(const rq::DelayHistory& h) {
    for (size_t j = 0; j < kFloats; ++j)
        if (std::memcmp(&h.ring[j], "\0\0\0\0", 4) != 0) return false;      // the bits: +0.0f
    return true;
}
static void scribble(rq::DelayHistory& h) { for (size_t j = 0; j < kFloats; ++j) h.ring[j] = 1.0f + (float)j; }

int main() {
    hipStream_t stream = nullptr;
    const uint32_t ids_a[kN] = {2, 0, 1, 2, 1}, ids_b[kN] = {0, 3, 3, 1, 2};
    Bank a, b;
    a.rows = 500; b.rows = 7;
    {
        Slot slot;
        rq::DelayHistory history;
        CHECK(history.ring.empty());
        // a first attach: the ring's allocation, its zeroing, then the slot's own allocation, upload and synchronise
        fake_hip::log.clear();
        CHECK(!history.attach(stream, slot, &a, ids_a, kN, kLd, kFloats));
        CHECK(fake_hip::log == "MZMUS" && history.ring.count() == kFloats && all_zero(history));
        CHECK(slot.bank == &a && a.attached == 1 && slot.gen != 0);
        const float* const block = history.ring.get();
        const uint64_t gen_a = slot.gen;
        // commands were written; a second attach (another bank) allocates nothing, keeps the block and zeroes it again
        scribble(history);
        fake_hip::log.clear();
        CHECK(!history.attach(stream, slot, &b, ids_b, kN, kLd, kFloats));
        CHECK(fake_hip::log == "ZUS" && history.ring.get() == block && all_zero(history));
        CHECK(slot.bank == &b && a.attached == 0 && b.attached == 1 && slot.gen != gen_a);
        // re-attaching the same bank zeroes too
        scribble(history);
        CHECK(!history.attach(stream, slot, &b, ids_b, kN, kLd, kFloats) && all_zero(history) && b.attached == 1);
        // detaching leaves the block for the next attachment, which zeroes it
        scribble(history);
        slot.detach();
        CHECK(history.ring.get() == block && slot.bank == nullptr && b.attached == 0);
        CHECK(!history.attach(stream, slot, &a, ids_a, kN, kLd, kFloats) && history.ring.get() == block && all_zero(history));
        // a zeroing that fails: returned, nothing after it, slot and banks as they were
        const uint64_t gen = slot.gen;
        fake_hip::log.clear();
        fail_next_memset = true;
        FirstRowsStatus failed = history.attach(stream, slot, &b, ids_b, kN, kLd, kFloats);
        CHECK(failed && failed.what == FirstRowsStatus::zero && failed.hip == hipErrorInvalidValue && fake_hip::log == "Z");
        CHECK(slot.bank == &a && slot.gen == gen && a.attached == 1 && b.attached == 0);
        CHECK(slot.ids.size() == kN && std::memcmp(slot.ids.data(), ids_a, sizeof(ids_a)) == 0);
        // a copy that fails: returned, slot and banks as they were (the history, zeroed before the copy, reads as zero)
        fake_hip::log.clear();
        fake_hip::fail_copy_in = 1;
        failed = history.attach(stream, slot, &b, ids_b, kN, kLd, kFloats);
        CHECK(failed && failed.what == FirstRowsStatus::copy && fake_hip::log == "ZU");
        CHECK(slot.bank == &a && slot.gen == gen && a.attached == 1 && b.attached == 0 && all_zero(history));
    }
    CHECK(a.attached == 0 && b.attached == 0);
    {   // a failing allocation of the ring: returned, no ring, the empty slot stays empty; the next attach makes it
        Slot slot;
        rq::DelayHistory history;
        fake_hip::log.clear();
        fake_hip::fail_allocation_in = 1;
        const FirstRowsStatus failed = history.attach(stream, slot, &a, ids_a, kN, kLd, kFloats);
        CHECK(failed && failed.what == FirstRowsStatus::device_allocation && fake_hip::log == "M");
        CHECK(history.ring.empty() && slot.bank == nullptr && slot.gen == 0 && slot.row0.empty() && a.attached == 0);
        // ... of the slot's first rows, behind a ring that was made: the ring stays for the next attachment
        fake_hip::log.clear();
        fake_hip::fail_allocation_in = 2;
        CHECK(history.attach(stream, slot, &a, ids_a, kN, kLd, kFloats).what == FirstRowsStatus::device_allocation);
        CHECK(fake_hip::log == "MZM" && !history.ring.empty() && slot.bank == nullptr && a.attached == 0);
        fake_hip::log.clear();
        CHECK(!history.attach(stream, slot, &a, ids_a, kN, kLd, kFloats) && fake_hip::log == "ZMUS" && a.attached == 1);
    }
    CHECK(a.attached == 0);
    CHECK(fake_hip::live() == 0 && fake_hip::bad_frees == 0);      // every block freed exactly once
    CHECK(memsets == 8);
    std::printf("ok\n");
    return 0;
}
