// rq_fused_route.hpp - which kernel flies a fused rollout: the family of the kernel text and the actor build, from what the launch
// description says (rq_kernels.hpp FusedArgs, fused_traits).  The one place that states the policy; launch_rollout_fused switches on
// its answer.  Host code without a HIP dependency: a plain host compiler takes this file alone (tests/route_driver.cpp does, and
// holds every row of the tables below against tests/test_routes_cpu.py's own copy).
#pragma once
#include <stdint.h>

#include "../../include/raptor_quad.h"

namespace rq {

// envs that fill the device at one wave per SIMD: 1024 SIMDs x 64 lanes
constexpr uint32_t kOneWavePerSimdEnvs = 65536u;

// The schedules an env can carry, in kind order: wrench, vehicle, wind, delay, sensor (rq_objects.hpp kTableKinds).  In fused mode
// each has one kernel family of its own - k_rollout_fused_<kind>, stamped from rq_rollout_schedule.inc - which serves a policy and a
// bank, tracked or not, at every native interval; the other families fly the launches without a schedule.
enum class FusedFamily { UNSUPPORTED, PLAIN, TRACK, RATE, BANK, BANK_RATE, WRENCH, VEHICLE, WIND, DELAY, SENSOR };
enum class FusedBuild { F32, F32_LEAN, BF16, F16X2 };      // ActorF32, ActorF32Lean, ActorBF16, ActorF16X2

struct FusedTraits {
    uint32_t n;             // envs
    int precision;          // rq_policy_precision
    bool sas;               // a SampleAndSquash stage is on
    bool tracked;           // a moving setpoint
    bool wrench;            // the env carries a wrench schedule
    uint32_t interval;      // one policy: its native interval
    bool bank;              // a policy bank acts ...
    bool bank_rated;        // ... and one of its intervals is above 1
    bool vehicle = false;   // the env carries a vehicle schedule
    bool wind = false;      // the env carries a wind schedule
    bool delay = false;     // the env carries a delay schedule
    bool sensor = false;    // the env carries a sensor schedule
};

struct FusedRoute { FusedFamily family; FusedBuild build; };

constexpr FusedRoute route_fused(const FusedTraits& t) {
    const bool f32 = t.precision == RQ_POLICY_FP32, bf16 = t.precision == RQ_POLICY_BF16_MFMA, f16x2 = t.precision == RQ_POLICY_F16X2_MFMA;
    // the schedules the env carries, in kind order: the enumerators from WRENCH on
    const bool carried[] = {t.wrench, t.vehicle, t.wind, t.delay, t.sensor};
    constexpr int kinds = sizeof(carried) / sizeof(carried[0]);
    static_assert((int)FusedFamily::SENSOR - (int)FusedFamily::WRENCH == kinds - 1, "one family per kind, in kind order");
    int schedules = 0, kind = 0;
    for (int k = 0; k < kinds; ++k)
        if (carried[k]) { ++schedules; kind = k; }
    // What no kernel is built for (the C layer refuses each before anything is enqueued): more than one schedule in fused mode; a
    // schedule beside a 16-bit policy or a SampleAndSquash stage; that stage anywhere but in the PLAIN family; a bank in anything but
    // fp32.
    const bool unsupported = !(f32 || bf16 || f16x2) || schedules > 1 || (schedules == 1 && (!f32 || t.sas)) ||
                             (t.sas && (t.tracked || t.bank || t.interval > 1)) || (t.bank && !f32);
    if (unsupported) return {FusedFamily::UNSUPPORTED, FusedBuild::F32};
    // A schedule's family serves one policy (tables null, single_interval = its interval) and a bank (tables set, single_interval = 1)
    // alike; TRACK is a template bool of RATE, BANK_RATE and the schedules' families, SAS one of PLAIN.
    const FusedFamily family = schedules == 1 ? (FusedFamily)((int)FusedFamily::WRENCH + kind)
                               : t.bank ? (t.tracked || t.bank_rated ? FusedFamily::BANK_RATE : FusedFamily::BANK)
                               : t.interval > 1 ? FusedFamily::RATE
                               : t.tracked ? FusedFamily::TRACK
                                           : FusedFamily::PLAIN;
    // The 16-bit actors have one build each, at every batch size.  fp32 has two builds of the same loop (same arithmetic, GRU two
    // tiles at a time): a 512-register one for one wave per SIMD - every batch up to 65 536 envs (1024 SIMDs x 64 lanes) - and a
    // 256-register one, two waves per SIMD, beyond.  The 256-register build parks loop invariants in scratch before the loop (~7 us
    // per launch); at one wave per SIMD both run the loop at the same speed (3.21 vs 3.23 us/step), so the small batches take the
    // build with the cheaper prologue.  With the SampleAndSquash stage: only the 256-register build carries it.
    const FusedBuild build = bf16 ? FusedBuild::BF16
                             : f16x2 ? FusedBuild::F16X2
                             : ((family == FusedFamily::PLAIN && t.sas) || t.n > kOneWavePerSimdEnvs) ? FusedBuild::F32_LEAN
                                                                                                      : FusedBuild::F32;
    return {family, build};
}

}  // namespace rq
