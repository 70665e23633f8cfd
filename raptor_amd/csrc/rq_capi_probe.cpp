// rq_capi_probe.cpp - reading the quadrotor out of the GRU state, behind the C ABI: the state entering every recorded step in the
// learner layout (rq_trajectory_get_hidden) and the second moments of [1, h_t, y] per bucket of episode age
// (rq_trajectory_probe_moments); the 17 x 17 solve per bucket that follows is the caller's, in float64 (raptor_amd/probing.py).
// Both read the saved state of a forward by this policy from the learned initial state at its current weights: the one a learner call
// left, or the state-only forward run here (grad_saved_initial, rq_capi_grad.cpp).  Kernels: rq_probe.hip.
#include <cmath>

#include "rq_objects.hpp"
#include "rq_probe.hpp"

using namespace rqh;

namespace {

int check_memory(int memory) {
    RQ_REQUIRE(memory >= RQ_DST_HOST && memory <= RQ_DST_DEVICE_ASYNC, RQ_ERR_INVALID_ARGUMENT, "memory must be 0, 1 or 2");
    return RQ_OK;
}

// a device-memory call's array: device memory of the trajectory's device
int check_device_array(const rq_device* dev, const void* p, const char* what, const char* name) {
    hipPointerAttribute_t at{};
    const hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) (void)hipGetLastError();
    RQ_REQUIRE(e == hipSuccess && at.type == hipMemoryTypeDevice && at.device == dev->ordinal, RQ_ERR_SHAPE_MISMATCH,
               std::string(what) + ": " + name + " lives on another device (or on the host): device memory of the trajectory's device is expected");
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
    if (memory != RQ_DST_HOST) { rc = check_device_array(dev, out, what, "out"); if (rc) return rc; }
    DeviceScope on_device(dev); rc = on_device.rc; if (rc) return rc;
    rc = grad_saved_initial(t, pol); if (rc) return rc;
    const size_t floats = (size_t)t->length * env->n * RQ_POLICY_HIDDEN_DIM;
    float* d_out = out;
    if (memory == RQ_DST_HOST) {
        RQ_HIP(t->grad.rows.reserve(dev->stream, floats));
        d_out = t->grad.rows;
    }
    RQ_HIP(rq::launch_probe_hidden_rows(dev->stream, env->n, env->ld, t->length, t->grad.saved, d_out));
    if (memory == RQ_DST_HOST) RQ_HIP(hipMemcpyAsync(out, d_out, floats * sizeof(float), hipMemcpyDeviceToHost, dev->stream));
    if (memory != RQ_DST_DEVICE_ASYNC) RQ_HIP(hipStreamSynchronize(dev->stream));
    return RQ_OK;
}

RQ_API int rq_trajectory_probe_moments(rq_trajectory* t, rq_policy* pol, const float* targets, uint32_t ld_targets, uint32_t n_targets,
                                       const uint32_t* age_edges, uint32_t n_buckets, double* moments, uint64_t* counts, int memory) {
    const char* what = "rq_trajectory_probe_moments";
    int rc = grad_check_pair(t, pol, what); if (rc) return rc;
    rc = check_memory(memory); if (rc) return rc;
    RQ_REQUIRE(targets, RQ_ERR_INVALID_ARGUMENT, "null argument: targets");
    RQ_REQUIRE(age_edges, RQ_ERR_INVALID_ARGUMENT, "null argument: age_edges");
    RQ_REQUIRE(moments, RQ_ERR_INVALID_ARGUMENT, "null argument: moments");
    RQ_REQUIRE(counts, RQ_ERR_INVALID_ARGUMENT, "null argument: counts");
    RQ_REQUIRE(n_targets >= 1 && n_targets <= rq::kProbeMaxTargets, RQ_ERR_INVALID_ARGUMENT,
               "n_targets must be 1 .. 15, not " + std::to_string(n_targets));
    RQ_REQUIRE(n_buckets >= 1 && n_buckets <= rq::kProbeMaxBuckets, RQ_ERR_INVALID_ARGUMENT,
               "n_buckets must be 1 .. 32, not " + std::to_string(n_buckets));
    rq::ProbeEdges edges{};
    for (uint32_t b = 0; b <= n_buckets; ++b) {
        RQ_REQUIRE(b == 0 || age_edges[b] > age_edges[b - 1], RQ_ERR_INVALID_ARGUMENT,
                   "age_edges must ascend strictly (age_edges[" + std::to_string(b) + "] does not)");
        edges.v[b] = age_edges[b];
    }
    rq_env* env = t->env;
    rq_device* dev = env->dev;
    RQ_REQUIRE(ld_targets >= env->n, RQ_ERR_INVALID_ARGUMENT, "ld_targets must be at least the number of envs");
    if (memory == RQ_DST_HOST) {
        for (uint32_t m = 0; m < n_targets; ++m)
            for (uint32_t i = 0; i < env->n; ++i)
                RQ_REQUIRE(std::isfinite(targets[(size_t)m * ld_targets + i]), RQ_ERR_INVALID_ARGUMENT,
                           "targets must be finite (target " + std::to_string(m) + ", env " + std::to_string(i) + " is not)");
    } else {
        rc = check_device_array(dev, targets, what, "targets"); if (rc) return rc;
        rc = check_device_array(dev, moments, what, "moments"); if (rc) return rc;
        rc = check_device_array(dev, counts, what, "counts"); if (rc) return rc;
    }
    DeviceScope on_device(dev); rc = on_device.rc; if (rc) return rc;
    rc = grad_saved_initial(t, pol); if (rc) return rc;
    RQ_HIP(t->grad.probe.reserve(dev->stream, rq::probe_partial_floats(env->n, n_buckets)));
    const size_t moment_doubles = (size_t)n_buckets * rq::kProbeDim * rq::kProbeDim;
    const float* d_y = targets;
    double* d_moments = moments;
    unsigned long long* d_counts = reinterpret_cast<unsigned long long*>(counts);
    if (memory == RQ_DST_HOST) {          // one device block: moments | counts | targets
        const size_t y_floats = (size_t)n_targets * ld_targets;
        RQ_HIP(t->grad.probe_io.reserve(dev->stream, moment_doubles + n_buckets + (y_floats + 1) / 2));
        d_moments = t->grad.probe_io;
        d_counts = reinterpret_cast<unsigned long long*>(d_moments + moment_doubles);
        float* y_dev = reinterpret_cast<float*>(d_moments + moment_doubles + n_buckets);
        RQ_HIP(hipMemcpyAsync(y_dev, targets, y_floats * sizeof(float), hipMemcpyHostToDevice, dev->stream));
        d_y = y_dev;
    }
    RQ_HIP(rq::launch_probe_moments(dev->stream, env->n, env->ld, t->length, t->grad.saved, t->done, d_y, ld_targets, n_targets, edges,
                                    n_buckets, t->grad.probe, d_moments, d_counts));
    if (memory == RQ_DST_HOST) {
        RQ_HIP(hipMemcpyAsync(moments, d_moments, moment_doubles * sizeof(double), hipMemcpyDeviceToHost, dev->stream));
        RQ_HIP(hipMemcpyAsync(counts, d_counts, (size_t)n_buckets * sizeof(uint64_t), hipMemcpyDeviceToHost, dev->stream));
    }
    if (memory != RQ_DST_DEVICE_ASYNC) RQ_HIP(hipStreamSynchronize(dev->stream));
    return RQ_OK;
}

}  // extern "C"
