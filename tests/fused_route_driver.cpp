// fused_route_driver.cpp - rq::route_fused (raptor_amd/csrc/rq_fused_route.hpp) under a plain host compiler: one line per row of the
// grid n x precision x SampleAndSquash x tracked x interval x actor x wrench, "n precision sas tracked interval actor wrench family
// build".  actor: 0 a policy, 1 a bank whose intervals are all 1, 2 a bank with an interval above 1.  Driven by
// tests/test_capi_cpu.py, which holds the expected answer of every row.
#include <cstdio>

#include "rq_fused_route.hpp"

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

int main() {
    const unsigned ns[] = {1u, 64u, 65536u, 65537u, 70001u};
    const int precisions[] = {RQ_POLICY_FP32, RQ_POLICY_BF16_MFMA, RQ_POLICY_F16X2_MFMA};
    for (unsigned n : ns)
        for (int precision : precisions)
            for (int sas = 0; sas < 2; ++sas)
                for (int tracked = 0; tracked < 2; ++tracked)
                    for (unsigned interval = 1; interval <= 2; ++interval)
                        for (int actor = 0; actor < 3; ++actor)
                            for (int wrench = 0; wrench < 2; ++wrench) {
                                const rq::FusedRoute r = rq::route_fused({n, precision, sas != 0, tracked != 0, wrench != 0, interval,
                                                                          actor != 0, actor == 2});
                                const bool ok = r.family != rq::FusedFamily::UNSUPPORTED;
                                std::printf("%u %d %d %d %u %d %d %s %s\n", n, precision, sas, tracked, interval, actor, wrench,
                                            name(r.family), ok ? name(r.build) : "-");
                            }
    return 0;
}
