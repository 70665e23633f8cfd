// env_schedule_driver.cpp - TESTS ONLY: rq::EnvSchedule and rq::upload_first_rows (raptor_amd/csrc/rq_env_schedule.hpp), the slot an
// env keeps per kind of schedule, against the counting stand-in of fake_hip_memory.cpp.  Prints "ok" and returns 0, or names the
// first check that failed.
#include <cstdio>
#include <cstring>
#include <memory>

#include "../raptor_amd/csrc/rq_env_schedule.hpp"
#include "fake_hip_memory.hpp"

using fake_hip::counters;
using rq::FirstRowsStatus;

#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) { std::printf("FAILED line %d: %s (calls so far: %s)\n", __LINE__, #cond, fake_hip::log.c_str()); return 1; } \
    } while (0)

// what a slot needs of a bank
struct Bank { uint32_t rows = 0, attached = 0; };
using Slot = rq::EnvSchedule<Bank>;
// an env as far as its schedules go: three slots, as rq_env holds them
struct Env { Slot schedule[3]; };

constexpr uint32_t kN = 5, kLd = 64;

// the [kLd] first rows on the "device": id * rows for i < n, 0 behind them (null ids: 0 everywhere)
static bool rows_are(const Slot& s, const uint32_t* ids, uint32_t rows) {
    for (uint32_t i = 0; i < kLd; ++i)
        if (s.row0[i] != (ids && i < kN ? ids[i] * rows : 0u)) return false;
    return true;
}

int main() {
    hipStream_t stream = nullptr;
    const uint32_t ids_a[kN] = {2, 0, 1, 2, 1}, ids_b[kN] = {0, 3, 3, 1, 2};
    Bank a, b;
    a.rows = 500; b.rows = 7;
    {
        Slot slot;
        CHECK(slot.bank == nullptr && slot.gen == 0 && slot.ids.empty() && slot.row0.empty());
        // (a) a first attach: one device allocation, one upload, one synchronise - in that order, and nothing else
        fake_hip::log.clear();
        counters = fake_hip::Counters{};
        CHECK(!slot.attach(stream, &a, ids_a, kN, kLd));
        CHECK(fake_hip::log == "MUS" && counters.total() == 3 && fake_hip::last_bytes == kLd * sizeof(uint32_t));
        // (b) the first rows; (c) the count; the ids as given
        CHECK(rows_are(slot, ids_a, a.rows));
        CHECK(slot.bank == &a && a.attached == 1 && slot.ids.size() == kN && std::memcmp(slot.ids.data(), ids_a, sizeof(ids_a)) == 0);
        const uint64_t gen_a = slot.gen;
        const uint32_t* const block = slot.row0.get();
        CHECK(gen_a != 0);
        // a second attach, of another bank: no allocation, the same block; the first bank is let go
        fake_hip::log.clear();
        CHECK(!slot.attach(stream, &b, ids_b, kN, kLd));
        CHECK(fake_hip::log == "US" && slot.row0.get() == block);
        CHECK(rows_are(slot, ids_b, b.rows));
        CHECK(slot.bank == &b && a.attached == 0 && b.attached == 1 && std::memcmp(slot.ids.data(), ids_b, sizeof(ids_b)) == 0);
        // (d) another attachment, another number
        const uint64_t gen_b = slot.gen;
        CHECK(gen_b != 0 && gen_b != gen_a);
        // null ids: table 0 for every env
        CHECK(!slot.attach(stream, &b, nullptr, kN, kLd));
        CHECK(rows_are(slot, nullptr, b.rows) && b.attached == 1 && slot.ids.size() == kN && slot.ids[1] == 0 && slot.gen != gen_b);
        // (e) a failing copy: returned, and slot and banks as before the call
        CHECK(!slot.attach(stream, &a, ids_a, kN, kLd));
        const uint64_t gen = slot.gen;
        fake_hip::log.clear();
        fake_hip::fail_copy_in = 1;
        const FirstRowsStatus failed = slot.attach(stream, &b, ids_b, kN, kLd);
        CHECK(failed && failed.what == FirstRowsStatus::copy && failed.hip == hipErrorInvalidValue && fake_hip::log == "U");
        CHECK(slot.bank == &a && slot.gen == gen && a.attached == 1 && b.attached == 0);
        CHECK(slot.ids.size() == kN && std::memcmp(slot.ids.data(), ids_a, sizeof(ids_a)) == 0 && rows_are(slot, ids_a, a.rows));
        // (c) detach: the count, the number, the ids; the block stays for the next attachment
        fake_hip::log.clear();
        slot.detach();
        CHECK(slot.bank == nullptr && slot.gen == 0 && slot.ids.empty() && a.attached == 0 && fake_hip::log.empty());
        CHECK(slot.row0.get() == block);
        slot.detach();      // nothing attached: nothing happens
        CHECK(a.attached == 0);
    }
    {   // (e) a failing allocation (only a first attachment allocates): returned, the empty slot stays empty, both banks' counts stay;
        // a failing copy at a first attachment leaves the block for the next
        Slot slot;
        fake_hip::log.clear();
        fake_hip::fail_allocation_in = 1;
        const FirstRowsStatus failed = slot.attach(stream, &a, ids_a, kN, kLd);
        CHECK(failed && failed.what == FirstRowsStatus::device_allocation && fake_hip::log == "M");
        CHECK(slot.bank == nullptr && slot.gen == 0 && slot.ids.empty() && slot.row0.empty() && a.attached == 0 && b.attached == 0);
        fake_hip::fail_copy_in = 1;
        CHECK(slot.attach(stream, &a, ids_a, kN, kLd).what == FirstRowsStatus::copy);
        CHECK(slot.bank == nullptr && slot.gen == 0 && slot.ids.empty() && a.attached == 0);
        fake_hip::log.clear();
        CHECK(!slot.attach(stream, &a, ids_a, kN, kLd) && fake_hip::log == "US" && a.attached == 1);
        // ... and another slot's failed allocation does not touch a bank this one holds
        Slot other;
        fake_hip::fail_allocation_in = 1;
        CHECK(other.attach(stream, &a, ids_b, kN, kLd).what == FirstRowsStatus::device_allocation);
        CHECK(a.attached == 1 && b.attached == 0 && other.bank == nullptr);
    }
    CHECK(a.attached == 0 && b.attached == 0);           // the slots went: their banks are let go
    {   // upload_first_rows alone (a reference bank's rows go through it): the same rows, one upload, one synchronise
        rq::DeviceBuffer<uint32_t> dst;
        CHECK(dst.alloc(kLd) == hipSuccess);
        fake_hip::log.clear();
        CHECK(!rq::upload_first_rows(stream, ids_b, kN, kLd, 9, dst) && fake_hip::log == "US");
        for (uint32_t i = 0; i < kLd; ++i) CHECK(dst[i] == (i < kN ? ids_b[i] * 9u : 0u));
    }
    {   // (f) an env that goes with three attached slots lets all three banks go
        Bank c;
        c.rows = 3;
        auto env = std::make_unique<Env>();
        CHECK(!env->schedule[0].attach(stream, &a, ids_a, kN, kLd) && !env->schedule[1].attach(stream, &b, nullptr, kN, kLd) &&
              !env->schedule[2].attach(stream, &c, ids_a, kN, kLd));
        CHECK(a.attached == 1 && b.attached == 1 && c.attached == 1);
        CHECK(env->schedule[0].gen != env->schedule[1].gen && env->schedule[1].gen != env->schedule[2].gen);
        env.reset();
        CHECK(a.attached == 0 && b.attached == 0 && c.attached == 0);
    }
    // (g)
    CHECK(fake_hip::live() == 0 && fake_hip::bad_frees == 0);
    std::printf("ok\n");
    return 0;
}
