// actor_step_route_driver.cpp - rq::route_actor_step (raptor_amd/csrc/rq_step_launch.hpp) under a plain host compiler: one line per
// row of the grid n x precision x actor x interval x mailbox x SampleAndSquash x hidden_in x forced groups per wave x leading
// dimension, "n precision actor interval mailbox sas hidden_in forced ld family build groups_per_wave grid".  actor: 0 a policy, 1 a
// bank, 2 a bank with its interval table.  ld: 0 = the batch rounded up to whole waves, else max(ld_h, ld_obs) itself.  Every row
// goes through an ActorStepLaunch and actor_step_traits, as the launcher's do.  Driven by tests/test_capi_cpu.py, which holds the
// expected answer of every row.
#include <cstdio>

#include "rq_step_launch.hpp"

static const char* name(rq::ActorFamily f) {
    switch (f) {
    case rq::ActorFamily::UNSUPPORTED: return "UNSUPPORTED";
    case rq::ActorFamily::STEP: return "STEP";
    case rq::ActorFamily::STREAM: return "STREAM";
    case rq::ActorFamily::RATE: return "RATE";
    case rq::ActorFamily::BANK: return "BANK";
    case rq::ActorFamily::BANK_RATE: return "BANK_RATE";
    }
    return "?";
}

static const char* name(rq::ActorBuild b) {
    switch (b) {
    case rq::ActorBuild::F32_LEAN: return "ActorF32Lean";
    case rq::ActorBuild::BF16: return "ActorBF16";
    case rq::ActorBuild::F16X2: return "ActorF16X2";
    }
    return "?";
}

int main() {
    const unsigned ns[] = {1u, 64u, 65u, 1023u, 1024u, 65536u, 262143u, 262144u, 2097152u};
    const int precisions[] = {RQ_POLICY_FP32, RQ_POLICY_BF16_MFMA, RQ_POLICY_F16X2_MFMA};
    const unsigned intervals[] = {1u, 3u}, forced_gpws[] = {0u, 4u};
    const unsigned lds[] = {0u, 20648881u, 20648882u};      // 104 ld bytes: the last below 2^31 - 1, the first at or above it
    static float f32[1];                                     // addresses to set the pointers with: nothing reads them
    static uint32_t u32[1];
    for (unsigned n : ns)
        for (int precision : precisions)
            for (int actor = 0; actor < 3; ++actor)
                for (unsigned interval : intervals)
                    for (int mailbox = 0; mailbox < 2; ++mailbox)
                        for (int sas = 0; sas < 2; ++sas)
                            for (int hidden_in = 0; hidden_in < 2; ++hidden_in)
                                for (unsigned forced : forced_gpws)
                                    for (unsigned ld : lds) {
                                        rq::ActorStepLaunch a;
                                        a.n = n; a.precision = precision; a.interval = interval;
                                        if (actor == 0) a.packed = f32;
                                        else { a.images = f32; a.block_policy = u32; }
                                        if (actor == 2) a.policy_interval = u32;
                                        if (mailbox) { a.mb.rows_in = f32; a.mb.rows_out = f32; a.mb.flag = u32; }
                                        if (sas) a.sas.mode = RQ_SAS_MEAN;
                                        if (hidden_in) a.hidden_in = f32;
                                        // the two leading dimensions the stream kernel's offsets depend on, the larger in either place
                                        const unsigned ld_max = ld ? ld : (n + 63u) / 64u * 64u;
                                        a.ld_h = hidden_in ? ld_max : 64u; a.ld_obs = hidden_in ? 64u : ld_max;
                                        const rq::ActorStepRoute r = rq::route_actor_step(rq::actor_step_traits(a, forced));
                                        const bool ok = r.family != rq::ActorFamily::UNSUPPORTED;
                                        std::printf("%u %d %d %u %d %d %d %u %u %s %s %u %u\n", n, precision, actor, interval, mailbox, sas,
                                                    hidden_in, forced, ld, name(r.family), ok ? name(r.build) : "-", r.groups_per_wave, r.grid);
                                    }
    return 0;
}
