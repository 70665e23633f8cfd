// rq_flight_launch.hpp - what one flight-table launch is (FlightTableLaunch; launch_trajectory_flight_table, rq_probe.hip, reads it
// and the C layer, rq_capi_probe.cpp, fills it): the recording's four fields, the age every env starts at, the buckets, the
// tolerance and the three outputs with the one statement of where a cell lies (flight_sum_cell, flight_peak_cell,
// flight_count_cell - the kernel stores by them, the tests' driver holds them).  flight_launch_refusal says why a description must
// not be launched: anything that would let a lane touch memory beside its own column.  Host code without a HIP dependency: a plain
// host compiler takes this file alone (tests/flight_launch_driver.cpp does).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/raptor_quad.h"

namespace rq {

constexpr uint32_t kFlightMaxBuckets = 32;      // the probe's (rq_probe.hpp kProbeMaxBuckets)

// One launch: a lane per env walks its column of the recording from t = 0 to steps - 1 and leaves, per bucket of episode age, nine
// sums, three peaks and a count (include/raptor_quad.h, "Flight table").  Set the fields by name.
struct FlightTableLaunch {
    uint32_t n = 0, ld = 0, steps = 0;
    // the recording: obs [steps][22][ld], act [steps][4][ld], rew [steps][ld], done [steps][ld]; columns below n <= ld are read
    const float* obs = nullptr;
    const float* act = nullptr;
    const float* rew = nullptr;
    const uint8_t* done = nullptr;
    const uint32_t* start = nullptr;                  // [n] on the device: the age of every env at step 0; null: 0
    float tol2 = 0.0f;                                // `outside` counts the steps with pos2 > tol2
    uint32_t n_buckets = 0;                           // 1 .. kFlightMaxBuckets
    uint32_t edges[kFlightMaxBuckets + 1] = {};       // edges[0 .. n_buckets], strictly ascending: bucket b holds ages [edges[b], edges[b + 1])
    // sum [n_buckets][RQ_FLIGHT_SUMS][ld_out], peak [n_buckets][RQ_FLIGHT_PEAKS][ld_out], count [n_buckets][ld_out], ld_out >= n:
    // every cell with column < n is written, columns >= n are left
    float* sum = nullptr;
    float* peak = nullptr;
    uint32_t* count = nullptr;
    uint32_t ld_out = 0;
};

constexpr size_t flight_sum_cell(uint32_t bucket, uint32_t column, uint32_t env, uint32_t ld_out) {
    return ((size_t)bucket * RQ_FLIGHT_SUMS + column) * ld_out + env;
}
constexpr size_t flight_peak_cell(uint32_t bucket, uint32_t column, uint32_t env, uint32_t ld_out) {
    return ((size_t)bucket * RQ_FLIGHT_PEAKS + column) * ld_out + env;
}
constexpr size_t flight_count_cell(uint32_t bucket, uint32_t env, uint32_t ld_out) { return (size_t)bucket * ld_out + env; }

// null: the description may be launched; else what is wrong with it
inline const char* flight_launch_refusal(const FlightTableLaunch& a) {
    if (a.n == 0 || a.steps == 0) return "no envs or no steps";
    if (!a.obs || !a.act || !a.rew || !a.done) return "a field of the recording is null";
    if (!a.sum || !a.peak || !a.count) return "an output is null";
    if (a.ld < a.n) return "ld < n";
    if (a.ld_out < a.n) return "ld_out < n";
    if (a.n_buckets < 1 || a.n_buckets > kFlightMaxBuckets) return "n_buckets outside 1 .. 32";
    for (uint32_t b = 1; b <= a.n_buckets; ++b)
        if (a.edges[b] <= a.edges[b - 1]) return "edges do not ascend strictly";
    return nullptr;
}

}  // namespace rq
