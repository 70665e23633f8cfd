// rq_capi_grad.cpp - the learner half of distillation (README.md:208-216) behind the C ABI: the fp32 student over a recorded
// trajectory (rq_trajectory_policy_forward) and the exact gradient of those actions with respect to its 2 084 parameters, back
// through time along the recorded episode structure (rq_trajectory_policy_backward).  Kernels: rq_grad.hpp.
#include "rq_objects.hpp"

using namespace rqh;

namespace {

// what both directions refuse: only the fp32 student without input or output stages has a gradient here
int check_pair(rq_trajectory* t, rq_policy* pol, const char* what) {
    RQ_REQUIRE(t && pol, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(pol->dev == t->env->dev, RQ_ERR_SHAPE_MISMATCH, std::string(what) + ": the policy lives on another device");
    RQ_REQUIRE(t->length > 0, RQ_ERR_INVALID_ARGUMENT, std::string(what) + ": the trajectory is empty");
    RQ_REQUIRE(pol->precision == RQ_POLICY_FP32, RQ_ERR_INVALID_ARGUMENT,
               std::string(what) + ": defined for the fp32 policy only (set_precision(RQ_POLICY_FP32)), not bf16 or f16x2");
    RQ_REQUIRE(!pol->standardize, RQ_ERR_INVALID_ARGUMENT,
               std::string(what) + ": the Standardize stage has no gradient here (disable it)");
    RQ_REQUIRE(pol->sas_mode == RQ_SAS_OFF, RQ_ERR_INVALID_ARGUMENT,
               std::string(what) + ": the SampleAndSquash stage has no gradient here (RQ_SAS_OFF)");
    return RQ_OK;
}

int check_memory(int memory) {
    RQ_REQUIRE(memory >= RQ_DST_HOST && memory <= RQ_DST_DEVICE_ASYNC, RQ_ERR_INVALID_ARGUMENT, "memory must be 0, 1 or 2");
    return RQ_OK;
}

}  // namespace

extern "C" {

RQ_API int rq_trajectory_policy_forward(rq_trajectory* t, rq_policy* pol, int start, float* action, uint32_t ld_action,
                                        int memory) {
    int rc = check_pair(t, pol, "rq_trajectory_policy_forward"); if (rc) return rc;
    rc = check_memory(memory); if (rc) return rc;
    RQ_REQUIRE(action, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(start == RQ_GRAD_START_CURRENT || start == RQ_GRAD_START_INITIAL, RQ_ERR_INVALID_ARGUMENT,
               "start must be RQ_GRAD_START_CURRENT or RQ_GRAD_START_INITIAL");
    rq_env* env = t->env;
    rq_device* dev = env->dev;
    RQ_REQUIRE(ld_action >= env->n, RQ_ERR_INVALID_ARGUMENT, "ld_action must be at least the number of envs");
    DeviceScope on_device(dev); rc = on_device.rc; if (rc) return rc;
    const uint32_t T = t->length, ld = env->ld;
    if (start == RQ_GRAD_START_CURRENT) { rc = policy_size(pol, env->n); if (rc) return rc; }
    // the transposed image of the backward, packed once per weight version
    if (!pol->w_packed_grad || pol->grad_image_version != pol->weight_version) {
        std::vector<float> image;
        try { image.resize(rq::RQ_PACKED_GRAD_FLOATS); } catch (const std::bad_alloc&) {
            return fail(RQ_ERR_OUT_OF_MEMORY, "rq_trajectory_policy_forward: host allocation failed");
        }
        rq::pack_policy_grad(pol->w_eff, image.data());
        RQ_HIP(hipStreamSynchronize(dev->stream));
        RQ_HIP(pol->w_packed_grad.reserve(dev->stream, image.size()));
        RQ_HIP(hipMemcpy(pol->w_packed_grad, image.data(), image.size() * sizeof(float), hipMemcpyHostToDevice));
        pol->grad_image_version = pol->weight_version;
    }
    t->grad.valid = false;
    RQ_HIP(t->grad.saved.reserve(dev->stream, (size_t)T * RQ_POLICY_HIDDEN_DIM * ld));
    float* d_act = action;
    if (memory == RQ_DST_HOST) {
        RQ_HIP(t->grad.rows.reserve(dev->stream, (size_t)T * RQ_ACTION_DIM * ld_action));
        d_act = t->grad.rows;
    }
    RQ_HIP(rq::launch_policy_grad_forward(dev->stream, env->n, ld, T, pol->w_packed, t->obs, t->done,
                                          start == RQ_GRAD_START_CURRENT ? pol->hidden : nullptr, pol->ld,
                                          start == RQ_GRAD_START_INITIAL, d_act, ld_action, t->grad.saved));
    t->grad.valid = true;
    t->grad.policy = pol;
    t->grad.weight_version = pol->weight_version;
    t->grad.length = T;
    t->grad.start = start;
    if (memory == RQ_DST_HOST)            // the envs' columns only: the caller's columns n .. ld_action-1 stay as they were
        RQ_HIP(hipMemcpy2DAsync(action, (size_t)ld_action * sizeof(float), d_act, (size_t)ld_action * sizeof(float),
                                (size_t)env->n * sizeof(float), (size_t)T * RQ_ACTION_DIM, hipMemcpyDeviceToHost, dev->stream));
    if (memory != RQ_DST_DEVICE_ASYNC) RQ_HIP(hipStreamSynchronize(dev->stream));
    return RQ_OK;
}

RQ_API int rq_trajectory_policy_backward(rq_trajectory* t, rq_policy* pol, const float* grad_action, uint32_t ld_grad,
                                         float* grad_weights, float* grad_hidden_start, int memory) {
    int rc = check_pair(t, pol, "rq_trajectory_policy_backward"); if (rc) return rc;
    rc = check_memory(memory); if (rc) return rc;
    RQ_REQUIRE(grad_action && grad_weights, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(t->grad.valid && t->grad.policy == pol && t->grad.length == t->length, RQ_ERR_INVALID_ARGUMENT,
               "rq_trajectory_policy_backward: no matching forward (rq_trajectory_policy_forward with this policy on this "
               "recording first)");
    RQ_REQUIRE(t->grad.weight_version == pol->weight_version, RQ_ERR_INVALID_ARGUMENT,
               "rq_trajectory_policy_backward: the policy's weights changed since the forward (run the forward again)");
    RQ_REQUIRE(grad_hidden_start == nullptr || t->grad.start == RQ_GRAD_START_CURRENT, RQ_ERR_INVALID_ARGUMENT,
               "rq_trajectory_policy_backward: dL/dh_start exists for RQ_GRAD_START_CURRENT only");
    rq_env* env = t->env;
    rq_device* dev = env->dev;
    RQ_REQUIRE(ld_grad >= env->n, RQ_ERR_INVALID_ARGUMENT, "ld_grad must be at least the number of envs");
    DeviceScope on_device(dev); rc = on_device.rc; if (rc) return rc;
    const uint32_t T = t->length, ld = env->ld, waves = (env->n + 63) / 64;
    RQ_HIP(t->grad.partial.reserve(dev->stream, (size_t)waves * RQ_POLICY_NUM_WEIGHTS));
    const float* d_ga = grad_action;
    float* d_gw = grad_weights;
    float* d_gh = grad_hidden_start;
    const size_t ga_bytes = (size_t)T * RQ_ACTION_DIM * ld_grad * sizeof(float);
    const size_t gh_bytes = (size_t)RQ_POLICY_HIDDEN_DIM * ld * sizeof(float);
    const size_t gw_bytes = (size_t)RQ_POLICY_NUM_WEIGHTS * sizeof(float);
    if (memory == RQ_DST_HOST) {          // one device block: dL/da | dL/dtheta | dL/dh_start
        const size_t off_gw = (ga_bytes + 255) & ~(size_t)255, off_gh = off_gw + ((gw_bytes + 255) & ~(size_t)255);
        RQ_HIP(t->grad.rows.reserve(dev->stream, (off_gh + gh_bytes) / sizeof(float)));
        char* base = reinterpret_cast<char*>(t->grad.rows.get());
        RQ_HIP(hipMemcpyAsync(base, grad_action, ga_bytes, hipMemcpyHostToDevice, dev->stream));
        d_ga = reinterpret_cast<const float*>(base);
        d_gw = reinterpret_cast<float*>(base + off_gw);
        d_gh = grad_hidden_start ? reinterpret_cast<float*>(base + off_gh) : nullptr;
    }
    RQ_HIP(rq::launch_policy_grad_backward(dev->stream, env->n, ld, T, pol->w_packed, pol->w_packed_grad, t->obs, t->done,
                                           t->grad.saved, d_ga, ld_grad, t->grad.start == RQ_GRAD_START_INITIAL, d_gh,
                                           t->grad.partial, d_gw));
    if (memory == RQ_DST_HOST) {
        RQ_HIP(hipMemcpyAsync(grad_weights, d_gw, gw_bytes, hipMemcpyDeviceToHost, dev->stream));
        if (grad_hidden_start) RQ_HIP(hipMemcpyAsync(grad_hidden_start, d_gh, gh_bytes, hipMemcpyDeviceToHost, dev->stream));
    }
    if (memory != RQ_DST_DEVICE_ASYNC) RQ_HIP(hipStreamSynchronize(dev->stream));
    return RQ_OK;
}

}  // extern "C"
