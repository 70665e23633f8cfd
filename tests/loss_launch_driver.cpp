// loss_launch_driver.cpp - rq::loss_partial_layout (raptor_amd/csrc/rq_loss_launch.hpp) under a plain host compiler: one line per n
// and form, "n weighted waves floats partial wsum sse live" - the whole workspace in floats and the float offset of every per-wave
// region.  Driven by tests/test_capi_cpu.py, which holds the sizes it expects itself.
#include <cstdio>

#include "rq_loss_launch.hpp"

static_assert(rq::loss_partial_layout(65, true).waves == 2, "the layout is a constant expression");

int main() {
    const unsigned ns[] = {1u, 64u, 65u, 129u, 65536u, 65537u, 70001u};
    for (unsigned n : ns)
        for (int weighted = 0; weighted < 2; ++weighted) {
            const rq::LossPartialLayout l = rq::loss_partial_layout(n, weighted != 0);
            std::printf("%u %d %u %zu %zu %zu %zu %zu\n", n, weighted, l.waves, l.floats, l.partial, l.wsum, l.sse, l.live);
        }
    const rq::LossLaunch a;          // a description names a single, unweighted launch until its fields say otherwise
    return a.block_policy == nullptr && a.weight == nullptr && a.n == 0 ? 0 : 1;
}
