// route_driver.cpp - what rq::route_fused (raptor_amd/csrc/rq_fused_route.hpp) and rq::route_env_step
// (raptor_amd/csrc/rq_step_launch.hpp) choose, under a plain host compiler (and again as a stand-alone program under
// -fsanitize=address,undefined): one line per row of the two grids.
//   "fused n precision sas tracked interval actor wrench vehicle wind delay sensor -> family build"
//       actor: 0 a policy, 1 a bank whose intervals are all 1, 2 a bank with an interval above 1
//   "step rollout bank wrench vehicle mailbox wind delay sensor -> supported bank rollout wrench vehicle wind delay family"
//       (a sensor schedule adds no step kernel: the row with it must be the row without it)
// Driven by tests/test_routes_cpu.py, which holds the expected answer of every row.
#include <cstdio>

#include "rq_fused_route.hpp"
#include "rq_step_launch.hpp"

static const char* name(rq::FusedFamily f) {
    switch (f) {
    case rq::FusedFamily::UNSUPPORTED: return "UNSUPPORTED";
    case rq::FusedFamily::PLAIN: return "PLAIN";
    case rq::FusedFamily::TRACK: return "TRACK";
    case rq::FusedFamily::RATE: return "RATE";
    case rq::FusedFamily::BANK: return "BANK";
    case rq::FusedFamily::BANK_RATE: return "BANK_RATE";
    case rq::FusedFamily::WRENCH: return "WRENCH";
    case rq::FusedFamily::VEHICLE: return "VEHICLE";
    case rq::FusedFamily::WIND: return "WIND";
    case rq::FusedFamily::DELAY: return "DELAY";
    case rq::FusedFamily::SENSOR: return "SENSOR";
    }
    return "?";
}

static const char* name(rq::FusedBuild b) {
    switch (b) {
    case rq::FusedBuild::F32: return "ActorF32";
    case rq::FusedBuild::F32_LEAN: return "ActorF32Lean";
    case rq::FusedBuild::BF16: return "ActorBF16";
    case rq::FusedBuild::F16X2: return "ActorF16X2";
    }
    return "?";
}

static const char* name(rq::EnvStepFamily f) {
    switch (f) {
    case rq::EnvStepFamily::NONE: return "NONE";
    case rq::EnvStepFamily::WRENCH: return "WRENCH";
    case rq::EnvStepFamily::VEHICLE: return "VEHICLE";
    case rq::EnvStepFamily::WIND: return "WIND";
    case rq::EnvStepFamily::DELAY: return "DELAY";
    }
    return "?";
}

int main() {
    const unsigned ns[] = {1u, 64u, 65536u, 65537u, 70001u};
    const int precisions[] = {RQ_POLICY_FP32, RQ_POLICY_BF16_MFMA, RQ_POLICY_F16X2_MFMA};
    for (unsigned n : ns)
        for (int precision : precisions)
            for (int sas = 0; sas < 2; ++sas)
                for (int tracked = 0; tracked < 2; ++tracked)
                    for (unsigned interval = 1; interval <= 2; ++interval)
                        for (int actor = 0; actor < 3; ++actor)
                            for (int schedules = 0; schedules < 32; ++schedules) {
                                const int wrench = schedules >> 4 & 1, vehicle = schedules >> 3 & 1, wind = schedules >> 2 & 1;
                                const int delay = schedules >> 1 & 1, sensor = schedules & 1;
                                rq::FusedTraits t{n, precision, sas != 0, tracked != 0, wrench != 0, interval, actor != 0, actor == 2};
                                t.vehicle = vehicle != 0;
                                t.wind = wind != 0;
                                t.delay = delay != 0;
                                t.sensor = sensor != 0;
                                const rq::FusedRoute r = rq::route_fused(t);
                                const bool ok = r.family != rq::FusedFamily::UNSUPPORTED;
                                std::printf("fused %u %d %d %d %u %d %d %d %d %d %d %s %s\n", n, precision, sas, tracked, interval, actor,
                                            wrench, vehicle, wind, delay, sensor, name(r.family), ok ? name(r.build) : "-");
                            }
    // the env step: the pointers are only compared with null
    static const float table[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    static const uint8_t steps[1] = {1u};
    static const uint32_t ids[1] = {0u};
    static float buffer[4];
    for (int rollout = 0; rollout < 2; ++rollout)
        for (int bank = 0; bank < 2; ++bank)
            for (int wrench = 0; wrench < 2; ++wrench)
                for (int vehicle = 0; vehicle < 2; ++vehicle)
                    for (int mailbox = 0; mailbox < 2; ++mailbox)
                        for (int wind = 0; wind < 2; ++wind)
                            for (int delay = 0; delay < 2; ++delay)
                                for (int sensor = 0; sensor < 2; ++sensor) {
                                    rq::EnvStepLaunch e;
                                    e.rollout = rollout != 0;
                                    e.state = buffer; e.next_state = buffer;
                                    if (bank) e.block_policy = ids;
                                    if (wrench) e.wr.rows = table;
                                    if (vehicle) e.vh.rows = table;
                                    if (mailbox) e.mb.rows_in = table;
                                    if (wind) e.wd.rows = table;
                                    if (delay) e.dl.rows = steps;
                                    if (sensor) { e.sn.rows = steps; e.sn.row0 = ids; e.sn.ring = buffer; e.sn.n_rows = 1; }
                                    const rq::EnvStepRoute r = rq::route_env_step(e);
                                    std::printf("step %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %s\n", rollout, bank, wrench, vehicle, mailbox,
                                                wind, delay, sensor, r.supported ? 1 : 0, r.bank ? 1 : 0, r.rollout ? 1 : 0, r.wrench ? 1 : 0,
                                                r.vehicle ? 1 : 0, r.wind ? 1 : 0, r.delay ? 1 : 0, name(r.family));
                                }
    static_assert(rq::kDelaySlots == 2 * RQ_DELAY_MAX_STEPS && (rq::kDelaySlots & (rq::kDelaySlots - 1u)) == 0, "the command ring's shape");
    static_assert(rq::kSensorSlots == 32 && rq::kSensorFields == 18 && rq::kSensorSlots == 2 * RQ_SENSOR_MAX_STEPS, "the ring's shape");
    return 0;
}
