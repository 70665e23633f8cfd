// rq_fused_route.hpp - which kernel flies a fused rollout: the family of the kernel text and the actor build, from what the launch
// description says (rq_kernels.hpp FusedArgs, fused_traits).  The one place that states the policy; launch_rollout_fused switches on
// its answer.  Host code without a HIP dependency: a plain host compiler takes this file alone (tests/fused_route_driver.cpp does,
// and holds every row of the tables below against tests/test_capi_cpu.py's own copy).
#pragma once
#include <stdint.h>

#include "../../include/raptor_quad.h"

namespace rq {

// envs that fill the device at one wave per SIMD: 1024 SIMDs x 64 lanes
constexpr uint32_t kOneWavePerSimdEnvs = 65536u;

enum class FusedFamily { UNSUPPORTED, PLAIN, TRACK, RATE, WRENCH, BANK, BANK_RATE };
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

// vehicle: the env carries a vehicle schedule - k_rollout_fused_vehicle flies the launch, whatever `family` (what the launch would be
// without the schedule) says; the entry point is one for a policy and a bank, tracked or not, at every native interval
// wind: likewise for a wind schedule and k_rollout_fused_wind; delay: for a delay schedule and k_rollout_fused_delay; sensor: for a
// sensor schedule and k_rollout_fused_sensor
struct FusedRoute { FusedFamily family; FusedBuild build; bool vehicle = false; bool wind = false; bool delay = false; bool sensor = false; };

constexpr FusedRoute route_fused(const FusedTraits& t) {
    const bool f32 = t.precision == RQ_POLICY_FP32, bf16 = t.precision == RQ_POLICY_BF16_MFMA, f16x2 = t.precision == RQ_POLICY_F16X2_MFMA;
    // What no kernel is built for (the C layer refuses each before anything is enqueued): a schedule beside a 16-bit policy or a
    // SampleAndSquash stage; that stage anywhere but in the PLAIN family; a bank in anything but fp32; a vehicle schedule beside a
    // 16-bit policy, that stage or a wrench schedule; a wind schedule beside a 16-bit policy, that stage or another schedule;
    // a delay schedule likewise; a sensor schedule likewise.
    const bool unsupported = !(f32 || bf16 || f16x2) || (t.wrench && (!f32 || t.sas)) ||
                             (t.sas && (t.tracked || t.bank || t.interval > 1)) || (t.bank && !f32) ||
                             (t.vehicle && (!f32 || t.sas || t.wrench)) || (t.wind && (!f32 || t.sas || t.wrench || t.vehicle)) ||
                             (t.delay && (!f32 || t.sas || t.wrench || t.vehicle || t.wind)) ||
                             (t.sensor && (!f32 || t.sas || t.wrench || t.vehicle || t.wind || t.delay));
    if (unsupported) return {FusedFamily::UNSUPPORTED, FusedBuild::F32, false, false, false, false};
    // WRENCH and the vehicle, wind and delay schedules' kernels serve one policy (tables null, single_interval = its interval) and a bank (tables set,
    // single_interval = 1) alike; TRACK is a template bool of RATE, BANK_RATE, WRENCH and the vehicle, wind and delay kernels, SAS one of PLAIN.
    const FusedFamily family = t.wrench ? FusedFamily::WRENCH
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
    return {family, build, t.vehicle, t.wind, t.delay, t.sensor};
}

}  // namespace rq
