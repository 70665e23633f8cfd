// rq_probe.hpp - what the host layer (rq_capi_probe.cpp) needs of rq_probe.hip: the second moments of z = [1, h_t, y] over the
// saved state of a recording, split by episode age; and the flight table, which reads the recording alone (rq_flight_launch.hpp).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "rq_flight_launch.hpp"

namespace rq {

constexpr uint32_t kProbeDim = 32;             // D: 1 + 16 hidden + up to 15 targets, zero-padded
constexpr uint32_t kProbeMaxTargets = 15;
constexpr uint32_t kProbeMaxBuckets = 32;

// the wave partials: S [waves][n_buckets][D][D] floats, then counts [waves][n_buckets] words
constexpr size_t probe_partial_floats(uint32_t n, uint32_t n_buckets) {
    return (size_t)((n + 63) / 64) * n_buckets * (kProbeDim * kProbeDim + 1);
}

// the age edges travel by value, as a kernel argument: edges v[0 .. n_buckets], strictly ascending
struct ProbeEdges { uint32_t v[kProbeMaxBuckets + 1]; };

// saved [steps][16][ld], done [steps][ld], y [n_targets][ld_y] or, `timed`, targets per step y [steps][n_targets][ld_y] (columns below
// n <= ld_y are read) -> moments [n_buckets][D][D] doubles (the full symmetric matrix) and counts [n_buckets].  Two launches:
// k_probe_moments or k_probe_moments_timed (a wave per 64 envs) and k_probe_reduce (the waves' partials in ascending wave order, in
// float64).  Deterministic: no atomics, every order fixed; timed targets that do not change over time give the untimed bits.
hipError_t launch_probe_moments(hipStream_t s, uint32_t n, uint32_t ld, uint32_t steps, const float* saved, const uint8_t* done,
                                const float* y, uint32_t ld_y, uint32_t n_targets, const ProbeEdges& edges, uint32_t n_buckets,
                                float* partial, double* moments, unsigned long long* counts, bool timed);

// done [steps][ld], tab [..][6] (a wrench bank's rows), row0 / start [n] (the env's first row in tab, its episode step count at step 0),
// params [RQ_PARAM_DIM][ld] -> out [steps][6][ld_out] (columns below n are written): the scheduled wrench row of every step, 0.0f on
// frozen steps; scale: in N / N m through wrench_scales of the params (else the row as it is).
hipError_t launch_probe_wrench_targets(hipStream_t s, uint32_t n, uint32_t ld, uint32_t steps, const uint8_t* done, const float* tab,
                                       uint32_t rows, const uint32_t* row0, const uint32_t* start, bool scale, const float* params,
                                       float gravity, float* out, uint32_t ld_out);

// One pass over the recording, a lane per env: sum / peak / count per bucket of episode age (FlightTableLaunch).  A description that
// would let a lane touch memory beside its column - ld_out < n, ld < n, n_buckets outside 1 .. 32, edges that do not ascend strictly,
// a null pointer (`start` may be null) - is refused with hipErrorInvalidValue and nothing is launched.  Deterministic: no atomics.
hipError_t launch_trajectory_flight_table(hipStream_t s, const FlightTableLaunch& a);

// saved [steps][16][ld] -> out [steps][n][16], the learner layout
hipError_t launch_probe_hidden_rows(hipStream_t s, uint32_t n, uint32_t ld, uint32_t steps, const float* saved, float* out);

}  // namespace rq
