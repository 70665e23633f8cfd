// flight_launch_driver.cpp - rq_flight_launch.hpp's FlightTableLaunch under a plain host compiler, with the address and undefined-
// behaviour sanitizers (tests/test_flight_table_cpu.py): a description nobody filled in names nothing and is refused; the refusals
// are the ones that keep a lane inside its own column; and the cell arithmetic covers [B][9 | 3 | 1][ld_out] exactly once, which the
// driver checks by marking every cell of arrays of exactly that size.  Exit status 0: all of it holds.
#include <cstdio>
#include <cstring>
#include <vector>

#include "rq_flight_launch.hpp"

int main() {
    int bad = 0;
    {
        const rq::FlightTableLaunch a;
        bad += a.n != 0 || a.ld != 0 || a.steps != 0 || a.n_buckets != 0 || a.ld_out != 0;
        bad += a.obs != nullptr || a.act != nullptr || a.rew != nullptr || a.done != nullptr || a.start != nullptr;
        bad += a.sum != nullptr || a.peak != nullptr || a.count != nullptr;
        bad += a.tol2 != 0.0f;
        for (uint32_t b = 0; b <= rq::kFlightMaxBuckets; ++b) bad += a.edges[b] != 0;
        bad += rq::flight_launch_refusal(a) == nullptr;          // refused rather than launched on leftovers
        static_assert(sizeof(a.edges) / sizeof(a.edges[0]) == rq::kFlightMaxBuckets + 1, "one edge more than buckets");
    }
    static_assert(rq::kFlightMaxBuckets == 32, "the probe's limit");
    static_assert(RQ_FLIGHT_SUMS == 9 && RQ_FLIGHT_PEAKS == 3, "nine sums, three peaks");
    static_assert(RQ_FLIGHT_POS2 == 0 && RQ_FLIGHT_TILT == 3 && RQ_FLIGHT_REWARD == 8 && RQ_FLIGHT_PEAK_OMEGA2 == 2, "the header's order");

    // a good description, then each way of spoiling it
    const uint32_t n = 130, ld = 192, ld_out = 137, B = 5;
    std::vector<float> obs(1), sum((size_t)B * RQ_FLIGHT_SUMS * ld_out), peak((size_t)B * RQ_FLIGHT_PEAKS * ld_out);
    std::vector<uint32_t> count((size_t)B * ld_out);
    uint8_t done = 0;
    rq::FlightTableLaunch good;
    good.n = n; good.ld = ld; good.steps = 40;
    good.obs = good.act = good.rew = obs.data(); good.done = &done;
    good.n_buckets = B;
    const uint32_t edges[B + 1] = {0, 1, 2, 4, 9, 0xffffffffu};
    std::memcpy(good.edges, edges, sizeof(edges));
    good.sum = sum.data(); good.peak = peak.data(); good.count = count.data(); good.ld_out = ld_out;
    bad += rq::flight_launch_refusal(good) != nullptr;
    auto refused = [&](auto spoil) {
        rq::FlightTableLaunch a = good;
        spoil(a);
        return rq::flight_launch_refusal(a) != nullptr;
    };
    bad += !refused([](rq::FlightTableLaunch& a) { a.ld_out = a.n - 1; });
    bad += !refused([](rq::FlightTableLaunch& a) { a.ld = a.n - 1; });
    bad += !refused([](rq::FlightTableLaunch& a) { a.n_buckets = 0; });
    bad += !refused([](rq::FlightTableLaunch& a) { a.n_buckets = 33; });
    bad += !refused([](rq::FlightTableLaunch& a) { a.edges[3] = a.edges[2]; });
    bad += !refused([](rq::FlightTableLaunch& a) { a.edges[1] = 0; });
    bad += !refused([](rq::FlightTableLaunch& a) { a.obs = nullptr; });
    bad += !refused([](rq::FlightTableLaunch& a) { a.act = nullptr; });
    bad += !refused([](rq::FlightTableLaunch& a) { a.rew = nullptr; });
    bad += !refused([](rq::FlightTableLaunch& a) { a.done = nullptr; });
    bad += !refused([](rq::FlightTableLaunch& a) { a.sum = nullptr; });
    bad += !refused([](rq::FlightTableLaunch& a) { a.peak = nullptr; });
    bad += !refused([](rq::FlightTableLaunch& a) { a.count = nullptr; });
    bad += !refused([](rq::FlightTableLaunch& a) { a.n = 0; });
    bad += !refused([](rq::FlightTableLaunch& a) { a.steps = 0; });
    bad += refused([](rq::FlightTableLaunch& a) { a.start = nullptr; a.ld_out = a.n; a.ld = a.n; a.n_buckets = 32;
                                                 for (uint32_t b = 0; b <= 32; ++b) a.edges[b] = b; });

    // every cell of every env below ld_out exactly once, inside arrays of exactly [B][9 | 3 | 1][ld_out]: the sanitizer sees a step outside
    for (uint32_t b = 0; b < B; ++b)
        for (uint32_t e = 0; e < ld_out; ++e) {
            for (uint32_t c = 0; c < RQ_FLIGHT_SUMS; ++c) sum[rq::flight_sum_cell(b, c, e, ld_out)] += 1.0f;
            for (uint32_t c = 0; c < RQ_FLIGHT_PEAKS; ++c) peak[rq::flight_peak_cell(b, c, e, ld_out)] += 1.0f;
            count[rq::flight_count_cell(b, e, ld_out)] += 1u;
        }
    for (float v : sum) bad += v != 1.0f;
    for (float v : peak) bad += v != 1.0f;
    for (uint32_t v : count) bad += v != 1u;
    bad += rq::flight_sum_cell(B - 1, RQ_FLIGHT_SUMS - 1, ld_out - 1, ld_out) + 1 != sum.size();
    bad += rq::flight_peak_cell(B - 1, RQ_FLIGHT_PEAKS - 1, ld_out - 1, ld_out) + 1 != peak.size();
    bad += rq::flight_count_cell(B - 1, ld_out - 1, ld_out) + 1 != count.size();
    // and no 32-bit wrap: the last cell of the largest table a uint32 stride allows
    bad += rq::flight_sum_cell(31, 8, 0xfffffffeu, 0xffffffffu) != ((size_t)31 * 9 + 8) * 0xffffffffull + 0xfffffffeull;
    std::printf("%d %zu %zu %zu\n", bad, sum.size(), peak.size(), count.size());
    return bad ? 1 : 0;
}
