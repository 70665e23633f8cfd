// sensor_history_driver.cpp - TESTS ONLY: the two rings an env keeps - the delay schedule's command history and the sensor schedule's
// readings, two instances of rq::DelayHistory (raptor_amd/csrc/rq_env_schedule.hpp) beside two schedule slots - against the counting
// stand-in of fake_hip_memory.cpp.  Prints "ok" and returns 0, or names the first check that failed.
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
constexpr size_t kCommandFloats = 32 * 4 * kLd;       // slots x action fields x ld
constexpr size_t kReadingFloats = 32 * 18 * kLd;      // slots x observation fields x ld

static bool all_zero(const rq::DelayHistory& h, size_t floats) {
    for (size_t j = 0; j < floats; ++j)
        if (std::memcmp(&h.ring[j], "\0\0\0\0", 4) != 0) return false;      // the bits: +0.0f
    return true;
}
static void scribble(rq::DelayHistory& h, size_t floats, float base) { for (size_t j = 0; j < floats; ++j) h.ring[j] = base + (float)j; }
static bool scribbled(const rq::DelayHistory& h, size_t floats, float base) {
    for (size_t j = 0; j < floats; ++j)
        if (h.ring[j] != base + (float)j) return false;
    return true;
}

// what an env holds of the two kinds
struct Env {
    Slot delay, sensor;
    rq::DelayHistory commands, readings;
};

int main() {
    hipStream_t stream = nullptr;
    const uint32_t ids_a[kN] = {2, 0, 1, 2, 1}, ids_b[kN] = {0, 3, 3, 1, 2};
    Bank delays, sensors, other;
    delays.rows = 7; sensors.rows = 12; other.rows = 3;
    {
        Env env;
        CHECK(env.commands.ring.empty() && env.readings.ring.empty());
        // the sensor schedule first: its ring alone is made, of its own size
        fake_hip::log.clear();
        CHECK(!env.readings.attach(stream, env.sensor, &sensors, ids_a, kN, kLd, kReadingFloats));
        CHECK(fake_hip::log == "MZMUS" && env.readings.ring.count() == kReadingFloats && all_zero(env.readings, kReadingFloats));
        CHECK(env.commands.ring.empty() && env.delay.bank == nullptr && env.sensor.bank == &sensors && sensors.attached == 1);
        // the delay schedule beside it: another block of another size; the readings are not touched
        scribble(env.readings, kReadingFloats, 3.0f);
        fake_hip::log.clear();
        CHECK(!env.commands.attach(stream, env.delay, &delays, ids_b, kN, kLd, kCommandFloats));
        CHECK(fake_hip::log == "MZMUS" && env.commands.ring.count() == kCommandFloats && all_zero(env.commands, kCommandFloats));
        CHECK(env.commands.ring.get() != env.readings.ring.get() && env.readings.ring.count() == kReadingFloats);
        CHECK(scribbled(env.readings, kReadingFloats, 3.0f) && delays.attached == 1 && sensors.attached == 1);
        const float* const readings_block = env.readings.ring.get();
        const float* const commands_block = env.commands.ring.get();
        // attaching the sensor schedule again zeroes its ring - every attachment does - and leaves the commands alone
        scribble(env.commands, kCommandFloats, 5.0f);
        const uint64_t delay_gen = env.delay.gen, sensor_gen = env.sensor.gen;
        fake_hip::log.clear();
        CHECK(!env.readings.attach(stream, env.sensor, &sensors, ids_b, kN, kLd, kReadingFloats));
        CHECK(fake_hip::log == "ZUS" && env.readings.ring.get() == readings_block && all_zero(env.readings, kReadingFloats));
        CHECK(scribbled(env.commands, kCommandFloats, 5.0f) && env.delay.gen == delay_gen && env.sensor.gen != sensor_gen);
        CHECK(sensors.attached == 1 && delays.attached == 1);
        // ... and the other way round
        scribble(env.readings, kReadingFloats, 7.0f);
        CHECK(!env.commands.attach(stream, env.delay, &delays, ids_a, kN, kLd, kCommandFloats));
        CHECK(env.commands.ring.get() == commands_block && all_zero(env.commands, kCommandFloats) && scribbled(env.readings, kReadingFloats, 7.0f));
        // detaching keeps the block for the next attachment, which zeroes it
        env.sensor.detach();
        CHECK(env.readings.ring.get() == readings_block && env.sensor.bank == nullptr && sensors.attached == 0 && delays.attached == 1);
        CHECK(!env.readings.attach(stream, env.sensor, &other, ids_a, kN, kLd, kReadingFloats));
        CHECK(env.readings.ring.get() == readings_block && all_zero(env.readings, kReadingFloats) && other.attached == 1);
        // a zeroing that fails: returned, nothing after it; both slots, both rings' blocks and every bank's count as they were
        scribble(env.commands, kCommandFloats, 9.0f);
        const uint64_t gen = env.sensor.gen;
        fake_hip::log.clear();
        fail_next_memset = true;
        FirstRowsStatus failed = env.readings.attach(stream, env.sensor, &sensors, ids_b, kN, kLd, kReadingFloats);
        CHECK(failed && failed.what == FirstRowsStatus::zero && failed.hip == hipErrorInvalidValue && fake_hip::log == "Z");
        CHECK(env.sensor.bank == &other && env.sensor.gen == gen && other.attached == 1 && sensors.attached == 0);
        CHECK(env.sensor.ids.size() == kN && std::memcmp(env.sensor.ids.data(), ids_a, sizeof(ids_a)) == 0);
        CHECK(env.delay.bank == &delays && delays.attached == 1 && scribbled(env.commands, kCommandFloats, 9.0f));
        CHECK(env.readings.ring.get() == readings_block && env.commands.ring.get() == commands_block);
        // a copy that fails: likewise (the readings, zeroed before the copy, read as zero)
        fake_hip::log.clear();
        fake_hip::fail_copy_in = 1;
        failed = env.readings.attach(stream, env.sensor, &sensors, ids_b, kN, kLd, kReadingFloats);
        CHECK(failed && failed.what == FirstRowsStatus::copy && fake_hip::log == "ZU");
        CHECK(env.sensor.bank == &other && env.sensor.gen == gen && other.attached == 1 && sensors.attached == 0);
        CHECK(env.delay.bank == &delays && delays.attached == 1 && scribbled(env.commands, kCommandFloats, 9.0f));
        CHECK(all_zero(env.readings, kReadingFloats));
    }
    CHECK(delays.attached == 0 && sensors.attached == 0 && other.attached == 0);
    {   // a failing allocation of the readings beside a command history that stands: returned, no ring of readings, the commands kept
        Env env;
        CHECK(!env.commands.attach(stream, env.delay, &delays, ids_a, kN, kLd, kCommandFloats));
        scribble(env.commands, kCommandFloats, 2.0f);
        fake_hip::log.clear();
        fake_hip::fail_allocation_in = 1;
        const FirstRowsStatus failed = env.readings.attach(stream, env.sensor, &sensors, ids_a, kN, kLd, kReadingFloats);
        CHECK(failed && failed.what == FirstRowsStatus::device_allocation && fake_hip::log == "M");
        CHECK(env.readings.ring.empty() && env.sensor.bank == nullptr && env.sensor.gen == 0 && sensors.attached == 0);
        CHECK(env.delay.bank == &delays && delays.attached == 1 && scribbled(env.commands, kCommandFloats, 2.0f));
        fake_hip::log.clear();
        CHECK(!env.readings.attach(stream, env.sensor, &sensors, ids_a, kN, kLd, kReadingFloats) && fake_hip::log == "MZMUS");
        CHECK(env.readings.ring.count() == kReadingFloats && sensors.attached == 1);
    }
    CHECK(delays.attached == 0 && sensors.attached == 0);
    CHECK(fake_hip::live() == 0 && fake_hip::bad_frees == 0);      // every block freed exactly once
    CHECK(memsets == 9);
    std::printf("ok\n");
    return 0;
}
