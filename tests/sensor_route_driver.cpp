// sensor_route_driver.cpp - what rq::route_fused (raptor_amd/csrc/rq_fused_route.hpp) and rq::route_env_step
// (raptor_amd/csrc/rq_step_launch.hpp) choose for the description rows a sensor schedule adds, under a plain host compiler (and again
// as a stand-alone program under -fsanitize=address,undefined).
//   "fused n precision sas tracked interval actor wrench vehicle wind delay sensor -> family build vehicle_kernel wind_kernel
//    delay_kernel sensor_kernel"
//       actor: 0 a policy, 1 a bank whose intervals are all 1, 2 a bank with an interval above 1
//   "step rollout bank wrench vehicle mailbox wind delay sensor -> family rollout wrench wind_kernel delay_kernel"
//       (a sensor schedule adds no step kernel: the row with it must be the row without it)
// With the argument "legacy" it leaves the new members unset and prints the rows of tests/delay_route_driver.cpp in that driver's
// format: the two outputs must be the same text.  Driven by tests/test_sensor_cpu.py, which holds the expected answer of every row.
#include <cstdio>
#include <cstring>

#include "rq_fused_route.hpp"
#include "rq_step_launch.hpp"

static const char* name(rq::FusedFamily f) {
    switch (f) {
    case rq::FusedFamily::UNSUPPORTED: return "UNSUPPORTED";
    case rq::FusedFamily::PLAIN: return "PLAIN";
    case rq::FusedFamily::TRACK: return "TRACK";
    case rq::FusedFamily::RATE: return "RATE";
    case rq::FusedFamily::WRENCH: return "WRENCH";
    case rq::FusedFamily::BANK: return "BANK";
    case rq::FusedFamily::BANK_RATE: return "BANK_RATE";
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
    case rq::EnvStepFamily::UNSUPPORTED: return "UNSUPPORTED";
    case rq::EnvStepFamily::STEP: return "k_step";
    case rq::EnvStepFamily::WRENCH: return "k_step_wrench";
    case rq::EnvStepFamily::VEHICLE: return "k_step_vehicle";
    case rq::EnvStepFamily::BANK: return "k_step_bank";
    case rq::EnvStepFamily::BANK_WRENCH: return "k_step_bank_wrench";
    case rq::EnvStepFamily::BANK_VEHICLE: return "k_step_bank_vehicle";
    }
    return "?";
}

int main(int argc, char** argv) {
    const bool legacy = argc > 1 && std::strcmp(argv[1], "legacy") == 0;
    const int sensors = legacy ? 1 : 2;
    const unsigned ns[] = {64u, 65536u, 65537u};
    const int precisions[] = {RQ_POLICY_FP32, RQ_POLICY_BF16_MFMA, RQ_POLICY_F16X2_MFMA};
    for (unsigned n : ns)
        for (int precision : precisions)
            for (int sas = 0; sas < 2; ++sas)
                for (int tracked = 0; tracked < 2; ++tracked)
                    for (unsigned interval = 1; interval <= 2; ++interval)
                        for (int actor = 0; actor < 3; ++actor)
                            for (int wrench = 0; wrench < 2; ++wrench)
                                for (int vehicle = 0; vehicle < 2; ++vehicle)
                                    for (int wind = 0; wind < 2; ++wind)
                                        for (int delay = 0; delay < 2; ++delay)
                                            for (int sensor = 0; sensor < sensors; ++sensor) {
                                                rq::FusedTraits t{n, precision, sas != 0, tracked != 0, wrench != 0, interval, actor != 0, actor == 2};
                                                t.vehicle = vehicle != 0;
                                                t.wind = wind != 0;
                                                t.delay = delay != 0;
                                                if (!legacy) t.sensor = sensor != 0;
                                                const rq::FusedRoute r = rq::route_fused(t);
                                                const bool ok = r.family != rq::FusedFamily::UNSUPPORTED;
                                                if (legacy) {
                                                    if (r.sensor) return 2;
                                                    std::printf("fused %u %d %d %d %u %d %d %d %d %d %s %s %d %d %d\n", n, precision, sas, tracked,
                                                                interval, actor, wrench, vehicle, wind, delay, name(r.family),
                                                                ok ? name(r.build) : "-", r.vehicle ? 1 : 0, r.wind ? 1 : 0, r.delay ? 1 : 0);
                                                } else {
                                                    std::printf("fused %u %d %d %d %u %d %d %d %d %d %d %s %s %d %d %d %d\n", n, precision, sas,
                                                                tracked, interval, actor, wrench, vehicle, wind, delay, sensor, name(r.family),
                                                                ok ? name(r.build) : "-", r.vehicle ? 1 : 0, r.wind ? 1 : 0, r.delay ? 1 : 0,
                                                                r.sensor ? 1 : 0);
                                                }
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
                                for (int sensor = 0; sensor < sensors; ++sensor) {
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
                                    if (legacy) {
                                        std::printf("step %d %d %d %d %d %d %d %s %d %d %d %d\n", rollout, bank, wrench, vehicle, mailbox, wind,
                                                    delay, name(r.family), r.rollout ? 1 : 0, r.wrench ? 1 : 0, r.wind ? 1 : 0, r.delay ? 1 : 0);
                                    } else {
                                        std::printf("step %d %d %d %d %d %d %d %d %s %d %d %d %d\n", rollout, bank, wrench, vehicle, mailbox,
                                                    wind, delay, sensor, name(r.family), r.rollout ? 1 : 0, r.wrench ? 1 : 0, r.wind ? 1 : 0,
                                                    r.delay ? 1 : 0);
                                    }
                                }
    static_assert(rq::kSensorSlots == 32 && rq::kSensorFields == 18 && rq::kSensorSlots == 2 * RQ_SENSOR_MAX_STEPS, "the ring's shape");
    return 0;
}
