// gain_launch_driver.cpp - rq_loss_launch.hpp's GainTableLaunch under a plain host compiler (tests/test_gain_reference_cpu.py):
// a description nobody filled in names nothing - every pointer null, every size 0, all edges 0 - so that
// launch_policy_gain_table refuses it rather than launching on leftovers.  Exit status 0: the defaults hold.
#include <cstdio>

#include "rq_loss_launch.hpp"

int main() {
    const rq::GainTableLaunch a;
    int bad = 0;
    bad += a.sum != nullptr;
    bad += a.count != nullptr;
    bad += a.ld_out != 0;
    bad += a.n_buckets != 0;
    for (uint32_t b = 0; b <= rq::kErrorTableMaxBuckets; ++b) bad += a.edges[b] != 0;
    const rq::LossLaunch& p = a.pass;
    bad += p.n != 0 || p.ld != 0 || p.steps != 0 || p.ld_h != 0 || p.n_policies != 0;
    bad += p.packed != nullptr || p.gpacked != nullptr || p.block_policy != nullptr;
    bad += p.obs != nullptr || p.done != nullptr || p.hidden != nullptr || p.saved != nullptr || p.target != nullptr;
    bad += p.start_initial;
    static_assert(sizeof(a.edges) / sizeof(a.edges[0]) == rq::kErrorTableMaxBuckets + 1, "one edge more than buckets");
    static_assert(rq::kErrorTableMaxBuckets == 32, "the probe's limit");
    std::printf("%d %zu\n", bad, sizeof(a.edges) / sizeof(a.edges[0]));
    return bad ? 1 : 0;
}
