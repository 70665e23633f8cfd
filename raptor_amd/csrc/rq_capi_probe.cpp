// rq_capi_probe.cpp - reading the quadrotor out of the GRU state, behind the C ABI: the state entering every recorded step in the
// learner layout (rq_trajectory_get_hidden) and the second moments of [1, h_t, y] per bucket of episode age
// (rq_trajectory_probe_moments; rq_trajectory_probe_moments_timed with targets per step); the 17 x 17 solve per bucket that follows
// is the caller's, in float64 (raptor_amd/probing.py).  rq_trajectory_wrench_targets rebuilds such targets on the device: the
// scheduled wrench every env was flown with at every recorded step.  rq_trajectory_flight_table reads the recording alone - no
// policy, no saved state: deviation, tilt, rates, effort and reward per env and bucket of episode age.
// The first three read the saved state of a forward by this policy from the learned initial state at its current weights: the one a
// learner call left, or the state-only forward run here (grad_saved_initial, rq_capi_grad.cpp).  Like the learner's calls each goes
// through one rq::CallMemory (rq_call_memory.hpp): refusals, DeviceScope, prepare, in, launch, out, finish.  Kernels: rq_probe.hip.
#include <cmath>

#include "rq_objects.hpp"
#include "rq_probe.hpp"

using namespace rqh;

namespace {

// rq_trajectory_probe_moments (targets [n_targets][ld_targets]) and, `timed`, rq_trajectory_probe_moments_timed (targets
// [length][n_targets][ld_targets]): one set of refusals, one device block, one launch.  `what`: the entry point's name.
int probe_moments(const char* what, bool timed, rq_trajectory* t, rq_policy* pol, const float* targets, uint32_t ld_targets,
                  uint32_t n_targets, const uint32_t* age_edges, uint32_t n_buckets, double* moments, uint64_t* counts, int memory) {
    int rc = grad_check_pair(t, pol, what); if (rc) return rc;
    rc = check_memory(memory); if (rc) return rc;
    RQ_REFUSE(what, targets, RQ_ERR_INVALID_ARGUMENT, "null argument: targets");
    RQ_REFUSE(what, age_edges, RQ_ERR_INVALID_ARGUMENT, "null argument: age_edges");
    RQ_REFUSE(what, moments, RQ_ERR_INVALID_ARGUMENT, "null argument: moments");
    RQ_REFUSE(what, counts, RQ_ERR_INVALID_ARGUMENT, "null argument: counts");
    RQ_REFUSE(what, n_targets >= 1 && n_targets <= rq::kProbeMaxTargets, RQ_ERR_INVALID_ARGUMENT,
              "n_targets must be 1 .. 15, not " + std::to_string(n_targets));
    RQ_REFUSE(what, n_buckets >= 1 && n_buckets <= rq::kProbeMaxBuckets, RQ_ERR_INVALID_ARGUMENT,
              "n_buckets must be 1 .. 32, not " + std::to_string(n_buckets));
    rq::ProbeEdges edges{};
    for (uint32_t b = 0; b <= n_buckets; ++b) {
        RQ_REFUSE(what, b == 0 || age_edges[b] > age_edges[b - 1], RQ_ERR_INVALID_ARGUMENT,
                  "age_edges must ascend strictly (age_edges[" + std::to_string(b) + "] does not)");
        edges.v[b] = age_edges[b];
    }
    rq_env* env = t->env;
    rq_device* dev = env->dev;
    RQ_REFUSE(what, ld_targets >= env->n, RQ_ERR_INVALID_ARGUMENT, "ld_targets must be at least the number of envs");
    const uint32_t blocks = timed ? t->length : 1u;          // [n_targets][ld_targets] blocks of targets: one, or one per step
    CallMemory mem(memory, dev->stream, dev->ordinal);
    if (mem.host()) {
        for (uint32_t s = 0; s < blocks; ++s)
            for (uint32_t m = 0; m < n_targets; ++m)
                for (uint32_t i = 0; i < env->n; ++i)
                    RQ_REFUSE(what, std::isfinite(targets[((size_t)s * n_targets + m) * ld_targets + i]), RQ_ERR_INVALID_ARGUMENT,
                              "targets must be finite (" + (timed ? "step " + std::to_string(s) + ", " : std::string()) + "target " +
                                  std::to_string(m) + ", env " + std::to_string(i) + " is not)");
    } else {
        rc = check_device_array(mem, targets, what, "targets"); if (rc) return rc;
        rc = check_device_array(mem, moments, what, "moments"); if (rc) return rc;
        rc = check_device_array(mem, counts, what, "counts"); if (rc) return rc;
    }
    DeviceScope on_device(dev); rc = on_device.rc; if (rc) return rc;
    rc = grad_saved_initial(t, pol); if (rc) return rc;
    RQ_HIP_AS(what, t->grad.probe.reserve(dev->stream, rq::probe_partial_floats(env->n, n_buckets)));
    const size_t moment_doubles = (size_t)n_buckets * rq::kProbeDim * rq::kProbeDim, y_floats = (size_t)blocks * n_targets * ld_targets;
    double* s_moments = nullptr; unsigned long long* s_counts = nullptr; float* s_y = nullptr;
    if (mem.host()) {          // one device block: moments | counts | targets (targets per step: a block of their own)
        RQ_HIP_AS(what, t->grad.probe_io.reserve(dev->stream, moment_doubles + n_buckets + (timed ? 0 : (y_floats + 1) / 2)));
        if (timed) RQ_HIP_AS(what, t->grad.probe_targets.reserve(dev->stream, y_floats));
        s_moments = t->grad.probe_io;
        s_counts = reinterpret_cast<unsigned long long*>(s_moments + moment_doubles);
        s_y = timed ? t->grad.probe_targets.get() : reinterpret_cast<float*>(s_moments + moment_doubles + n_buckets);
    }
    const float* d_y = nullptr; RQ_HIP_AS(what, mem.in(targets, y_floats, s_y, &d_y));
    double* d_moments = mem.out(moments, moment_doubles, s_moments);
    unsigned long long* d_counts = mem.out(reinterpret_cast<unsigned long long*>(counts), n_buckets, s_counts);
    RQ_HIP_AS(what, rq::launch_probe_moments(dev->stream, env->n, env->ld, t->length, t->grad.saved, t->done, d_y, ld_targets, n_targets,
                                             edges, n_buckets, t->grad.probe, d_moments, d_counts, timed));
    RQ_HIP_AS(what, mem.finish());
    return RQ_OK;
}

}  // namespace

extern "C" {

RQ_API int rq_trajectory_get_hidden(rq_trajectory* t, rq_policy* pol, float* out, int memory) {
    const char* what = "rq_trajectory_get_hidden";
    int rc = grad_check_pair(t, pol, what); if (rc) return rc;
    rc = check_memory(memory); if (rc) return rc;
    RQ_REQUIRE(out, RQ_ERR_INVALID_ARGUMENT, "null argument: out");
    rq_env* env = t->env;
    rq_device* dev = env->dev;
    CallMemory mem(memory, dev->stream, dev->ordinal);
    rc = check_device_array(mem, out, what, "out"); if (rc) return rc;
    DeviceScope on_device(dev); rc = on_device.rc; if (rc) return rc;
    rc = grad_saved_initial(t, pol); if (rc) return rc;
    const size_t floats = (size_t)t->length * env->n * RQ_POLICY_HIDDEN_DIM;
    if (mem.host()) RQ_HIP(t->grad.rows.reserve(dev->stream, floats));
    float* d_out = mem.out(out, floats, t->grad.rows.get());
    RQ_HIP(rq::launch_probe_hidden_rows(dev->stream, env->n, env->ld, t->length, t->grad.saved, d_out));
    RQ_HIP(mem.finish());
    return RQ_OK;
}

RQ_API int rq_trajectory_probe_moments(rq_trajectory* t, rq_policy* pol, const float* targets, uint32_t ld_targets, uint32_t n_targets,
                                       const uint32_t* age_edges, uint32_t n_buckets, double* moments, uint64_t* counts, int memory) {
    return probe_moments(__func__, false, t, pol, targets, ld_targets, n_targets, age_edges, n_buckets, moments, counts, memory);
}

RQ_API int rq_trajectory_probe_moments_timed(rq_trajectory* t, rq_policy* pol, const float* targets, uint32_t ld_targets,
                                             uint32_t n_targets, const uint32_t* age_edges, uint32_t n_buckets, double* moments,
                                             uint64_t* counts, int memory) {
    return probe_moments(__func__, true, t, pol, targets, ld_targets, n_targets, age_edges, n_buckets, moments, counts, memory);
}

RQ_API int rq_trajectory_wrench_targets(rq_trajectory* t, const rq_wrench_bank* bank, const uint32_t* wrench_id, const rq_params* params,
                                        const uint32_t* start_steps, int units_out, float* out, uint32_t ld_out, int memory) {
    const char* what = __func__;
    RQ_REQUIRE(t, RQ_ERR_INVALID_ARGUMENT, "null argument: trajectory");
    RQ_REQUIRE(bank, RQ_ERR_INVALID_ARGUMENT, "null argument: bank");
    RQ_REQUIRE(params, RQ_ERR_INVALID_ARGUMENT, "null argument: params");
    RQ_REQUIRE(out, RQ_ERR_INVALID_ARGUMENT, "null argument: out");
    int rc = check_memory(memory); if (rc) return rc;
    rq_env* env = t->env;
    rq_device* dev = env->dev;
    const uint32_t n = env->n, limit = env->cfg.episode_step_limit;
    RQ_REQUIRE(t->length > 0, RQ_ERR_INVALID_ARGUMENT, "the trajectory is empty");
    RQ_REQUIRE(bank->dev == dev, RQ_ERR_SHAPE_MISMATCH, "the wrench bank lives on another device");
    RQ_REQUIRE(params->env == env, RQ_ERR_SHAPE_MISMATCH, "the params belong to another env than the trajectory");
    RQ_REQUIRE(units_out == RQ_WRENCH_RELATIVE || units_out == RQ_WRENCH_ABSOLUTE, RQ_ERR_INVALID_ARGUMENT,
               "unknown units_out: RQ_WRENCH_RELATIVE or RQ_WRENCH_ABSOLUTE");
    RQ_REQUIRE(!(units_out == RQ_WRENCH_RELATIVE && bank->units == RQ_WRENCH_ABSOLUTE), RQ_ERR_INVALID_ARGUMENT,
               "relative output from an absolute bank: its rows are N and N m (ask for RQ_WRENCH_ABSOLUTE)");
    RQ_REQUIRE(ld_out >= n, RQ_ERR_INVALID_ARGUMENT, "ld_out must be at least the number of envs");
    RQ_REQUIRE(bank->rows >= limit, RQ_ERR_INVALID_ARGUMENT,
               "the wrench bank has fewer rows (" + std::to_string(bank->rows) + ") than episode_step_limit (" + std::to_string(limit) +
                   "): every table must cover an episode");
    for (uint32_t i = 0; wrench_id && i < n; ++i)
        RQ_REQUIRE(wrench_id[i] < bank->n_tables, RQ_ERR_INVALID_ARGUMENT,
                   "wrench id out of range: env " + std::to_string(i) + " names table " + std::to_string(wrench_id[i]) + " of a bank of " +
                       std::to_string(bank->n_tables));
    for (uint32_t i = 0; start_steps && i < n; ++i)
        RQ_REQUIRE(start_steps[i] < limit, RQ_ERR_INVALID_ARGUMENT,
                   "start_steps out of range: env " + std::to_string(i) + " starts at episode step " + std::to_string(start_steps[i]) +
                       ", episode_step_limit is " + std::to_string(limit));
    CallMemory mem(memory, dev->stream, dev->ordinal);
    rc = check_device_array(mem, out, what, "out"); if (rc) return rc;
    DeviceScope on_device(dev); rc = on_device.rc; if (rc) return rc;

    // first rows | start steps go through the trajectory's pinned block and are uploaded only when they differ from the call
    // before: no wait for the stream then, and none at the first call
    rq_trajectory::Grad& g = t->grad;
    if (g.probe_rows_host.count() < 2 * (size_t)n) {
        if (!g.probe_rows_host.empty()) RQ_HIP(hipStreamSynchronize(dev->stream));      // a copy may still read the old block
        g.probe_rows_host.reset();
        g.probe_rows_valid = false;
        RQ_HIP(g.probe_rows_host.alloc(2 * (size_t)n));
    }
    RQ_HIP(g.probe_rows.reserve(dev->stream, 2 * (size_t)n));
    uint32_t* rows_host = g.probe_rows_host;
    bool same = g.probe_rows_valid;
    for (uint32_t i = 0; same && i < n; ++i)
        same = rows_host[i] == (wrench_id ? wrench_id[i] : 0u) * bank->rows && rows_host[n + i] == (start_steps ? start_steps[i] : 0u);
    if (!same) {
        if (g.probe_rows_valid) RQ_HIP(hipStreamSynchronize(dev->stream));
        g.probe_rows_valid = false;
        for (uint32_t i = 0; i < n; ++i) {
            rows_host[i] = (wrench_id ? wrench_id[i] : 0u) * bank->rows;          // < n_tables * rows < 2^28
            rows_host[n + i] = start_steps ? start_steps[i] : 0u;
        }
        RQ_HIP(hipMemcpyAsync(g.probe_rows, rows_host, 2 * (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, dev->stream));
        g.probe_rows_valid = true;
    }
    // a host-memory call: packed [length][6][n] on the device, only the envs' columns go back
    if (mem.host()) RQ_HIP(g.rows.reserve(dev->stream, (size_t)t->length * 6 * n));
    const uint32_t d_ld = mem.host() ? n : ld_out;
    float* d_out = mem.out(out, ld_out, g.rows.get(), n, n, (size_t)t->length * 6);
    const bool scale = units_out == RQ_WRENCH_ABSOLUTE && bank->units == RQ_WRENCH_RELATIVE;
    RQ_HIP(rq::launch_probe_wrench_targets(dev->stream, n, env->ld, t->length, t->done, bank->d, bank->rows, g.probe_rows,
                                           g.probe_rows.get() + n, scale, params->d, env->cfg.gravity, d_out, d_ld));
    RQ_HIP(mem.finish());
    return RQ_OK;
}

RQ_API int rq_trajectory_flight_table(rq_trajectory* t, const uint32_t* start_steps, float tolerance, const uint32_t* age_edges,
                                      uint32_t n_buckets, float* sum, float* peak, uint32_t* count, uint32_t ld_out, int memory) {
    const char* what = __func__;
    RQ_REQUIRE(t, RQ_ERR_INVALID_ARGUMENT, "null argument: trajectory");
    RQ_REQUIRE(age_edges, RQ_ERR_INVALID_ARGUMENT, "null argument: age_edges");
    RQ_REQUIRE(sum, RQ_ERR_INVALID_ARGUMENT, "null argument: sum");
    RQ_REQUIRE(peak, RQ_ERR_INVALID_ARGUMENT, "null argument: peak");
    RQ_REQUIRE(count, RQ_ERR_INVALID_ARGUMENT, "null argument: count");
    int rc = check_memory(memory); if (rc) return rc;
    rq_env* env = t->env;
    rq_device* dev = env->dev;
    const uint32_t n = env->n, B = n_buckets;
    RQ_REQUIRE(t->length > 0, RQ_ERR_INVALID_ARGUMENT, "the trajectory is empty");
    RQ_REQUIRE(ld_out >= n, RQ_ERR_INVALID_ARGUMENT, "ld_out must be at least the number of envs");
    RQ_REQUIRE(B >= 1 && B <= rq::kFlightMaxBuckets, RQ_ERR_INVALID_ARGUMENT, "n_buckets must be 1 .. 32, not " + std::to_string(B));
    rq::FlightTableLaunch a;
    for (uint32_t b = 0; b <= B; ++b) {
        RQ_REQUIRE(b == 0 || age_edges[b] > age_edges[b - 1], RQ_ERR_INVALID_ARGUMENT,
                   "age_edges must ascend strictly (age_edges[" + std::to_string(b) + "] does not)");
        a.edges[b] = age_edges[b];
    }
    a.n_buckets = B;
    RQ_REQUIRE(std::isfinite(tolerance) && tolerance >= 0.0f, RQ_ERR_INVALID_ARGUMENT, "tolerance must be finite and not negative");
    a.tol2 = tolerance * tolerance;
    CallMemory mem(memory, dev->stream, dev->ordinal);
    rc = check_device_array(mem, sum, what, "sum"); if (rc) return rc;
    rc = check_device_array(mem, peak, what, "peak"); if (rc) return rc;
    rc = check_device_array(mem, count, what, "count"); if (rc) return rc;
    DeviceScope on_device(dev); rc = on_device.rc; if (rc) return rc;

    // the start steps go through the trajectory's pinned block and are uploaded only when they differ from the call before
    rq_trajectory::Grad& g = t->grad;
    if (start_steps) {
        if (g.flight_start_host.count() < (size_t)n) {
            if (!g.flight_start_host.empty()) RQ_HIP(hipStreamSynchronize(dev->stream));      // a copy may still read the old block
            g.flight_start_host.reset();
            g.flight_start_valid = false;
            RQ_HIP(g.flight_start_host.alloc(n));
        }
        RQ_HIP(g.flight_start.reserve(dev->stream, n));
        uint32_t* host = g.flight_start_host;
        bool same = g.flight_start_valid;
        for (uint32_t i = 0; same && i < n; ++i) same = host[i] == start_steps[i];
        if (!same) {
            if (g.flight_start_valid) RQ_HIP(hipStreamSynchronize(dev->stream));
            g.flight_start_valid = false;
            for (uint32_t i = 0; i < n; ++i) host[i] = start_steps[i];
            RQ_HIP(hipMemcpyAsync(g.flight_start, host, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, dev->stream));
            g.flight_start_valid = true;
        }
        a.start = g.flight_start;
    }
    // a host-memory call: packed sum [B][9][n] | peak [B][3][n] | count [B][n] on the device, only the envs' columns go back
    const size_t sums = (size_t)B * RQ_FLIGHT_SUMS * n, peaks = (size_t)B * RQ_FLIGHT_PEAKS * n, counts = (size_t)B * n;
    float* s_sum = nullptr;
    if (mem.host()) {
        RQ_HIP(g.rows.reserve(dev->stream, sums + peaks + counts));
        s_sum = g.rows.get();
    }
    a.n = n; a.ld = env->ld; a.steps = t->length;
    a.obs = t->obs; a.act = t->act; a.rew = t->rew; a.done = t->done;
    a.sum = mem.out(sum, ld_out, s_sum, n, n, (size_t)B * RQ_FLIGHT_SUMS);
    a.peak = mem.out(peak, ld_out, s_sum ? s_sum + sums : nullptr, n, n, (size_t)B * RQ_FLIGHT_PEAKS);
    a.count = mem.out(count, ld_out, s_sum ? reinterpret_cast<uint32_t*>(s_sum + sums + peaks) : nullptr, n, n, (size_t)B);
    a.ld_out = mem.host() ? n : ld_out;
    RQ_HIP(rq::launch_trajectory_flight_table(dev->stream, a));
    RQ_HIP(mem.finish());
    return RQ_OK;
}

}  // extern "C"
