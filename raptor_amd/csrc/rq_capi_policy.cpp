// rq_capi_policy.cpp - foundation_policy.Raptor behind the C ABI (README.md:19-24,48,94,97; checkpoint.h:34-194): create, the optional
// Standardize / SampleAndSquash stages, reset, evaluate_step (with the small-batch loop's speculation hit), evaluate_sequence, selftest.
#include "rq_objects.hpp"

namespace rqh {

// precision in bits 0-7, bit 8 = tanh on the output (what the sequence / relabel launchers take)
int mode_of(const rq_policy* pol) { return pol->precision | ((pol->sas_mode != RQ_SAS_OFF ? 1 : 0) << 8); }

rq::SasArgs sas_of(const rq_policy* pol, uint32_t epoch, const uint32_t* epoch_base, uint64_t env_offset) {
    return {(uint32_t)pol->sas_mode, epoch, epoch_base, pol->ls_image, pol->sas_seed, env_offset};
}

const float* packed_of(const rq_policy* pol) {
    return pol->precision == RQ_POLICY_BF16_MFMA ? pol->w_packed_bf16
         : pol->precision == RQ_POLICY_F16X2_MFMA ? pol->w_packed_f16x2 : pol->w_packed;
}

// Size the per-batch buffers on first use (Raptor sizes its hidden state on the first
// batch, README.md:24) and apply a pending reset(): h <- initial_hidden_state.
int policy_size(rq_policy* pol, uint32_t batch) {
    DeviceScope on_device(pol->dev); int rc = on_device.rc; if (rc) return rc;
    pol->version = fresh_version();            // every user of the hidden state comes through here: a speculation based on it is void
    if (pol->batch != batch || !pol->hidden) {
        RQ_REQUIRE(pol->batch == 0 || pol->needs_reset, RQ_ERR_SHAPE_MISMATCH,
                   "batch size changed without reset (hidden state is per batch element)");
        RQ_HIP(hipStreamSynchronize(pol->dev->stream));
        pol->hidden.reset(); pol->hidden_alt.reset(); pol->obs.reset(); pol->act.reset();
        pol->batch = pol->ld = 0;                  // not sized, should an allocation below fail
        const uint32_t ld = round_up64(batch);
        RQ_HIP(pol->hidden.alloc((size_t)RQ_POLICY_HIDDEN_DIM * ld));
        RQ_HIP(pol->hidden_alt.alloc((size_t)RQ_POLICY_HIDDEN_DIM * ld));
        RQ_HIP(pol->obs.alloc((size_t)RQ_POLICY_INPUT_DIM * ld));
        RQ_HIP(pol->act.alloc((size_t)RQ_ACTION_DIM * ld));
        pol->batch = batch; pol->ld = ld;
        pol->needs_reset = true;
    }
    if (pol->needs_reset) {
        if (pol->mirror_stale)       // updated on the device: the initial state is read there, in stream order
            RQ_HIP(rq::launch_fill_rows(pol->dev->stream, pol->hidden, pol->ld, pol->w_dev + 2000, RQ_POLICY_HIDDEN_DIM));
        else
            for (int j = 0; j < RQ_POLICY_HIDDEN_DIM; ++j)
                RQ_HIP(rq::launch_fill_f32(pol->dev->stream, pol->hidden + (size_t)j * pol->ld,
                                           pol->w_host[2000 + j], pol->ld));
        pol->needs_reset = false;
    }
    return RQ_OK;
}

int policy_mirror(rq_policy* pol) {
    if (!pol->mirror_stale) return RQ_OK;
    DeviceScope on_device(pol->dev); int rc = on_device.rc; if (rc) return rc;
    RQ_HIP(hipMemcpyAsync(pol->w_host, pol->w_dev, sizeof(pol->w_host), hipMemcpyDeviceToHost, pol->dev->stream));
    RQ_HIP(hipStreamSynchronize(pol->dev->stream));
    std::memcpy(pol->w_eff, pol->w_host, sizeof(pol->w_eff));      // a device-side update is refused with a Standardize stage
    pol->mirror_stale = false;
    return RQ_OK;
}

int require_native_rate(const rq_policy* pol, const char* what) {
    RQ_REQUIRE(pol->native_interval == 1, RQ_ERR_INVALID_ARGUMENT,
               std::string(what) + ": defined at the native rate only, the policy's native interval is " +
                   std::to_string(pol->native_interval) + " (rq_policy_set_native_interval(policy, 1))");
    return RQ_OK;
}

// RQ_POLICY_F16X2_MFMA cannot hold a weight whose operand reaches 65 520 after the gate pre-scale (rq::policy_f16x2_misfit)
int refuse_f16x2_misfit(const float* w_eff, const char* who) {
    const int i = rq::policy_f16x2_misfit(w_eff);
    if (i < 0) return RQ_OK;
    char msg[256];
    std::snprintf(msg, sizeof msg, "%s: weight %d is outside the f16 range (magnitude >= 65520 after the gate pre-scale of -log2 e on the "
                  "r and z rows, -2 log2 e on the n rows): the f16x2 image cannot hold it, use fp32 or bf16", who, i);
    return fail(RQ_ERR_INVALID_ARGUMENT, msg);
}

int policy_images16(rq_policy* pol) {
    if (!pol->images16_stale) return RQ_OK;
    int rc = policy_mirror(pol); if (rc) return rc;
    std::vector<float> packed16, packed_split;
    try { packed16.resize(rq::RQ_PACKED_BF16_FLOATS); packed_split.resize(rq::RQ_PACKED_F16X2_FLOATS); } catch (const std::bad_alloc&) {
        return fail(RQ_ERR_OUT_OF_MEMORY, "policy images: host allocation failed");
    }
    rq::pack_policy_bf16(pol->w_eff, packed16.data());
    rq::pack_policy_f16x2(pol->w_eff, packed_split.data());
    DeviceScope on_device(pol->dev); rc = on_device.rc; if (rc) return rc;
    RQ_HIP(hipStreamSynchronize(pol->dev->stream));
    RQ_HIP(hipMemcpy(pol->w_packed_bf16, packed16.data(), packed16.size() * sizeof(float), hipMemcpyHostToDevice));
    RQ_HIP(hipMemcpy(pol->w_packed_f16x2, packed_split.data(), packed_split.size() * sizeof(float), hipMemcpyHostToDevice));
    pol->images16_stale = false;
    return RQ_OK;
}


}  // namespace rqh

using namespace rqh;

extern "C" {

// ---------------------------------------------------------------------------- Policy ----
// the parameters the kernels see: `weights` with the optional Standardize stage folded into layer_0
static void effective_weights(const rq_policy* p, const float* weights, float* eff) {
    std::memcpy(eff, weights, sizeof(float) * RQ_POLICY_NUM_WEIGHTS);
    if (!p->standardize) return;
    // Standardize (x - mean) / std followed by Dense folds into the Dense:
    //   W0' = W0 diag(1/std),  b0' = b0 - W0' mean      (semantics unpinned)
    for (int o = 0; o < 16; ++o) {
        float shift = 0.0f;
        for (int k = 0; k < RQ_POLICY_INPUT_DIM; ++k) {
            const float w = weights[o * 22 + k] * p->std_inv[k];
            eff[o * 22 + k] = w;
            shift += w * p->std_mean[k];
        }
        eff[352 + o] = weights[352 + o] - shift;
    }
}

// (re)build the effective parameters and both MFMA operand images, and upload them.  `weights`: the new raw parameters
// (p->w_host itself when only a stage changed).  A policy in RQ_POLICY_F16X2_MFMA refuses parameters its image cannot hold,
// and is then left exactly as it was.
static int policy_upload(rq_policy* p, const float* weights, const char* who) {
    float eff[RQ_POLICY_NUM_WEIGHTS];
    effective_weights(p, weights, eff);
    if (p->precision == RQ_POLICY_F16X2_MFMA) { const int rc = refuse_f16x2_misfit(eff, who); if (rc) return rc; }
    if (weights != p->w_host) std::memcpy(p->w_host, weights, sizeof(p->w_host));
    std::memcpy(p->w_eff, eff, sizeof(p->w_eff));
    p->version = fresh_version();
    p->weight_version = fresh_version();
    std::vector<float> packed, packed16, packed_split;
    try {                                   // nothing throws across the boundary
        packed.resize(rq::RQ_PACKED_FLOATS); packed16.resize(rq::RQ_PACKED_BF16_FLOATS); packed_split.resize(rq::RQ_PACKED_F16X2_FLOATS);
    } catch (const std::bad_alloc&) {
        return fail(RQ_ERR_OUT_OF_MEMORY, "policy upload: host allocation failed");
    }
    rq::pack_policy(p->w_eff, packed.data());
    rq::pack_policy_bf16(p->w_eff, packed16.data());
    rq::pack_policy_f16x2(p->w_eff, packed_split.data());
    DeviceScope on_device(p->dev); int rc = on_device.rc; if (rc) return rc;
    RQ_HIP(hipStreamSynchronize(p->dev->stream));
    RQ_HIP(hipMemcpy(p->w_dev, p->w_eff, sizeof(p->w_eff), hipMemcpyHostToDevice));
    RQ_HIP(hipMemcpy(p->w_packed, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice));
    RQ_HIP(hipMemcpy(p->w_packed_bf16, packed16.data(), packed16.size() * sizeof(float), hipMemcpyHostToDevice));
    RQ_HIP(hipMemcpy(p->w_packed_f16x2, packed_split.data(), packed_split.size() * sizeof(float), hipMemcpyHostToDevice));
    p->mirror_stale = p->images16_stale = false;
    return RQ_OK;
}

RQ_API int rq_policy_create(rq_device* dev, const float* weights, size_t n_weights, rq_policy** out) {
    RQ_REQUIRE(dev && weights && out, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(n_weights == RQ_POLICY_NUM_WEIGHTS, RQ_ERR_INVALID_ARGUMENT,
               "expected 2084 weights: W0[16,22] b0[16] Wi[48,16] Wh[48,16] bi[48] bh[48] h0[16] W2[4,16] b2[4]");
    *out = nullptr;
    DeviceScope on_device(dev); int rc = on_device.rc; if (rc) return rc;
    rq_policy* p = new (std::nothrow) rq_policy();
    RQ_REQUIRE(p, RQ_ERR_OUT_OF_MEMORY, "host allocation failed");
    p->dev = dev; p->ordinal = dev->ordinal;
    std::memcpy(p->w_host, weights, sizeof(p->w_host));
    if (p->w_dev.alloc(RQ_POLICY_NUM_WEIGHTS) != hipSuccess || p->w_packed.alloc(rq::RQ_PACKED_FLOATS) != hipSuccess ||
        p->w_packed_bf16.alloc(rq::RQ_PACKED_BF16_FLOATS) != hipSuccess || p->w_packed_f16x2.alloc(rq::RQ_PACKED_F16X2_FLOATS) != hipSuccess) {
        delete p;
        return fail(RQ_ERR_OUT_OF_MEMORY, "rq_policy_create: device allocation failed");
    }
    policy_registry(p, +1);
    rc = policy_upload(p, p->w_host, "rq_policy_create");
    if (rc) { rq_policy_destroy(p); return rc; }
    *out = p;
    return RQ_OK;
}

RQ_API int rq_policy_destroy(rq_policy* pol) {
    if (!pol) return RQ_OK;
    DeviceScope on_device(pol->ordinal);
    if (device_registry(pol->dev, 0)) (void)resident_retire(pol->dev);
    policy_registry(pol, -1);      // rq_device::spec.last_policy may still name this object: it is checked against the registry
    delete pol;
    return RQ_OK;
}

// New parameters for an existing policy: precision, the Standardize and SampleAndSquash stages and the hidden state stay; every
// path then computes what a policy created with these weights computes.  A resident executor bound to the device is retired first
// (it holds the old operands in registers), as rq_policy_destroy does.
RQ_API int rq_policy_set_weights(rq_policy* pol, const float* weights, size_t n_weights) {
    RQ_REQUIRE(pol && weights, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(n_weights == RQ_POLICY_NUM_WEIGHTS, RQ_ERR_INVALID_ARGUMENT,
               "expected 2084 weights: W0[16,22] b0[16] Wi[48,16] Wh[48,16] bi[48] bh[48] h0[16] W2[4,16] b2[4]");
    DeviceScope on_device(pol->dev); int rc = on_device.rc; if (rc) return rc;
    if (device_registry(pol->dev, 0)) { rc = resident_retire(pol->dev); if (rc) return rc; }
    return policy_upload(pol, weights, "rq_policy_set_weights");
}

RQ_API int rq_policy_get_weights(rq_policy* pol, float* host_out) {
    RQ_REQUIRE(pol && host_out, RQ_ERR_INVALID_ARGUMENT, "null argument");
    int rc = policy_mirror(pol); if (rc) return rc;
    std::memcpy(host_out, pol->w_host, sizeof(pol->w_host));
    return RQ_OK;
}

RQ_API int rq_policy_pack_image(const float* weights, size_t n_weights, int precision, float* image, size_t capacity,
                                size_t* floats) {
    RQ_REQUIRE(weights && floats, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(n_weights == RQ_POLICY_NUM_WEIGHTS, RQ_ERR_INVALID_ARGUMENT, "expected 2084 weights");
    RQ_REQUIRE(precision == RQ_POLICY_FP32 || precision == RQ_POLICY_BF16_MFMA || precision == RQ_POLICY_F16X2_MFMA,
               RQ_ERR_INVALID_ARGUMENT, "unknown precision");
    const size_t need = precision == RQ_POLICY_FP32 ? (size_t)rq::RQ_PACKED_FLOATS
                      : precision == RQ_POLICY_BF16_MFMA ? (size_t)rq::RQ_PACKED_BF16_FLOATS : (size_t)rq::RQ_PACKED_F16X2_FLOATS;
    *floats = need;
    if (!image) return RQ_OK;
    RQ_REQUIRE(capacity >= need, RQ_ERR_INVALID_ARGUMENT, "image buffer too small");
    if (precision == RQ_POLICY_FP32) rq::pack_policy(weights, image);
    else if (precision == RQ_POLICY_BF16_MFMA) rq::pack_policy_bf16(weights, image);
    else {
        const int rc = refuse_f16x2_misfit(weights, "rq_policy_pack_image"); if (rc) return rc;
        rq::pack_policy_f16x2(weights, image);
    }
    return RQ_OK;
}

RQ_API int rq_policy_set_precision(rq_policy* pol, int precision) {
    RQ_REQUIRE(pol, RQ_ERR_INVALID_ARGUMENT, "null argument");
    pol->version = fresh_version();
    RQ_REQUIRE(precision == RQ_POLICY_FP32 || precision == RQ_POLICY_BF16_MFMA || precision == RQ_POLICY_F16X2_MFMA,
               RQ_ERR_INVALID_ARGUMENT, "unknown precision");
    if (precision != RQ_POLICY_FP32) { int rc = policy_images16(pol); if (rc) return rc; }      // (fetches w_eff after a device-side update)
    if (precision == RQ_POLICY_F16X2_MFMA) { int rc = refuse_f16x2_misfit(pol->w_eff, "rq_policy_set_precision"); if (rc) return rc; }
    pol->precision = precision;
    return RQ_OK;
}

RQ_API int rq_policy_set_standardize(rq_policy* pol, const float* mean, const float* std) {
    RQ_REQUIRE(pol, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE((mean == nullptr) == (std == nullptr), RQ_ERR_INVALID_ARGUMENT, "mean and std must be given together");
    { int rc = policy_mirror(pol); if (rc) return rc; }
    if (mean)
        for (int k = 0; k < RQ_POLICY_INPUT_DIM; ++k) RQ_REQUIRE(std[k] > 0.0f, RQ_ERR_INVALID_ARGUMENT, "std must be positive");
    const bool was = pol->standardize;                 // a refused fold (f16x2 range) leaves the stage as it was
    float old_mean[RQ_POLICY_INPUT_DIM], old_inv[RQ_POLICY_INPUT_DIM];
    std::memcpy(old_mean, pol->std_mean, sizeof(old_mean));
    std::memcpy(old_inv, pol->std_inv, sizeof(old_inv));
    if (mean) {
        for (int k = 0; k < RQ_POLICY_INPUT_DIM; ++k) {
            pol->std_mean[k] = mean[k];
            pol->std_inv[k] = 1.0f / std[k];
        }
    }
    pol->standardize = mean != nullptr;
    const int rc = policy_upload(pol, pol->w_host, "rq_policy_set_standardize");
    if (rc == RQ_ERR_INVALID_ARGUMENT) {
        pol->standardize = was;
        std::memcpy(pol->std_mean, old_mean, sizeof(old_mean));
        std::memcpy(pol->std_inv, old_inv, sizeof(old_inv));
    }
    return rc;
}

RQ_API int rq_policy_set_squash(rq_policy* pol, int enable) {
    RQ_REQUIRE(pol, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(!enable || pol->native_interval == 1, RQ_ERR_INVALID_ARGUMENT,
               "the SampleAndSquash stage is not carried at a native interval above 1 (the policy's is " +
                   std::to_string(pol->native_interval) + ")");
    pol->version = fresh_version();
    pol->sas_mode = enable ? RQ_SAS_MEAN : RQ_SAS_OFF;
    return RQ_OK;
}

// The native interval R (include/raptor_quad.h): weights, precision and hidden state stay; the call counter starts again.  A resident
// executor bound to the device is retired first (it knows R = 1 only), as rq_policy_set_weights does.
RQ_API int rq_policy_set_native_interval(rq_policy* pol, uint32_t interval) {
    RQ_REQUIRE(pol, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(interval >= 1 && interval <= RQ_POLICY_MAX_NATIVE_INTERVAL, RQ_ERR_INVALID_ARGUMENT,
               "native interval " + std::to_string(interval) + " is outside 1 .. 64");
    RQ_REQUIRE(interval == 1 || pol->sas_mode == RQ_SAS_OFF, RQ_ERR_INVALID_ARGUMENT,
               "native interval " + std::to_string(interval) + ": an interval above 1 does not carry the SampleAndSquash stage (RQ_SAS_OFF)");
    DeviceScope on_device(pol->dev); int rc = on_device.rc; if (rc) return rc;
    if (device_registry(pol->dev, 0)) { rc = resident_retire(pol->dev); if (rc) return rc; }
    pol->version = fresh_version();
    pol->native_interval = interval;
    pol->rate_counter = 0;
    return RQ_OK;
}

RQ_API int rq_policy_get_native_interval(const rq_policy* pol, uint32_t* interval) {
    RQ_REQUIRE(pol && interval, RQ_ERR_INVALID_ARGUMENT, "null argument");
    *interval = pol->native_interval;
    return RQ_OK;
}

RQ_API int rq_policy_set_sample_and_squash(rq_policy* pol, int mode, const float* log_std_weights, const float* log_std_bias,
                                    uint64_t seed) {
    RQ_REQUIRE(pol, RQ_ERR_INVALID_ARGUMENT, "null argument");
    pol->version = fresh_version();
    RQ_REQUIRE(mode == RQ_SAS_OFF || mode == RQ_SAS_MEAN || mode == RQ_SAS_SAMPLE, RQ_ERR_INVALID_ARGUMENT, "unknown mode");
    RQ_REQUIRE(mode == RQ_SAS_OFF || pol->native_interval == 1, RQ_ERR_INVALID_ARGUMENT,
               "the SampleAndSquash stage is not carried at a native interval above 1 (the policy's is " +
                   std::to_string(pol->native_interval) + ")");
    if (mode == RQ_SAS_SAMPLE) {
        DeviceScope on_device(pol->dev); int rc = on_device.rc; if (rc) return rc;
        std::vector<float> image;
        try { image.resize(rq::RQ_LOGSTD_FLOATS); } catch (const std::bad_alloc&) { return fail(RQ_ERR_OUT_OF_MEMORY, "rq_policy_set_sample_and_squash: host allocation failed"); }
        rq::pack_logstd_head(log_std_weights, log_std_bias, image.data());
        RQ_HIP(hipStreamSynchronize(pol->dev->stream));
        RQ_HIP(pol->ls_image.reserve(pol->dev->stream, image.size()));
        RQ_HIP(hipMemcpy(pol->ls_image, image.data(), image.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    pol->sas_mode = mode;
    pol->sas_seed = seed;
    pol->sas_counter = 0;
    return RQ_OK;
}

RQ_API int rq_policy_reset(rq_policy* pol) {
    RQ_REQUIRE(pol, RQ_ERR_INVALID_ARGUMENT, "null argument");
    pol->version = fresh_version();
    DeviceScope on_device(pol->dev); int rc = on_device.rc; if (rc) return rc;
    pol->needs_reset = true;   // applied (h <- initial_hidden_state, checkpoint.h:123) on the next use
    pol->sas_counter = 0;
    pol->rate_counter = 0;     // the next call is native
    return RQ_OK;
}

RQ_API int rq_policy_evaluate_step(rq_policy* pol, rq_env* env, const float* observation, uint32_t batch,
                            uint32_t obs_stride, float* action) {
    RQ_REQUIRE(pol, RQ_ERR_INVALID_ARGUMENT, "null policy");
    RQ_REQUIRE(observation || env, RQ_ERR_INVALID_ARGUMENT, "observation == NULL needs an env to read from");
    RQ_REQUIRE(action || env, RQ_ERR_INVALID_ARGUMENT, "action == NULL needs an env to write to");
    if (env) {
        RQ_REQUIRE(env->dev == pol->dev, RQ_ERR_SHAPE_MISMATCH, "env and policy live on different devices");
        RQ_REQUIRE(batch == env->n, RQ_ERR_SHAPE_MISMATCH, "batch must equal the env's n_envs");
    }
    RQ_REQUIRE(batch > 0, RQ_ERR_INVALID_ARGUMENT, "batch must be positive");
    if (observation) RQ_REQUIRE(obs_stride >= RQ_POLICY_INPUT_DIM, RQ_ERR_INVALID_ARGUMENT, "obs_stride < 22");
    DeviceScope on_device(pol->dev, rq::KeepResident{}); int rc = on_device.rc; if (rc) return rc;
    rq_device* dev = pol->dev;
    const bool rated = pol->native_interval > 1;      // never speculated, never resident: plain launches of k_actor_step_rate
    if (observation && action && !env && batch < kGpuLayoutMinEnvs && !rated) {
        bool hit = false;
        rc = speculation_take(dev, pol, observation, batch, obs_stride, action, &hit); if (rc || hit) return rc;
    }
    // ---- the policy alone, at most 16 rows, called again and again (README.md:17-25: a caller with a simulator of its own): from the
    // third call in a row on - each within 200 us of the one before, nothing else asked of the device in between - the rows go to a
    // wave that stays on the device (k_resident_policy) instead of into a launch.  Same lifecycle as the loop's executor
    // (rq_resident.cpp): retired before anything else touches the device, replayed as a launch if it had left.
    ResidentExecutor& rx = dev->resident;
    const bool pol_eligible = rx.enabled && observation && action && !env && batch <= rq::kResidentPolicyBatch &&
                              pol->precision == RQ_POLICY_FP32 && pol->sas_mode == RQ_SAS_OFF && !rated;
    const uint64_t now_ns = pol_eligible ? host_now_ns() : 0;
    // in a row = the same policy at the same batch: two policies evaluated in turns (a student and a teacher on the same rows) would
    // otherwise retire each other's kernel call after call.  Stored below, once the call has gone the one way or the other.
    const uint32_t streak = rx.policy_streak.follow(pol_eligible, now_ns, pol, batch);
    const bool ready = pol_eligible && pol->batch == batch && pol->hidden && !pol->needs_reset;      // nothing to size or fill
    ResidentBinding want{};
    want.policy_kind = true; want.pol = pol; want.packed = packed_of(pol); want.batch = batch;
    want.hidden[0] = want.hidden[1] = pol->hidden;
    bool resident = false;
    rc = resident_admit(dev, ready, want, now_ns, streak, &resident); if (rc) return rc;
    if (resident) {
        rc = ensure_mailbox(dev); if (rc) return rc;
        if (!rx.running) {
            rq::ResidentArgs ra{};
            ra.b = rq::Batch{batch, pol->ld, 0}; ra.ld_h = pol->ld; ra.pol_act = pol->act;
            rc = resident_start(dev, ra, want); if (rc) return rc;
        }
        if (rx.running) {
            rc = mailbox_put_in(dev, observation, batch, RQ_POLICY_INPUT_DIM, obs_stride); if (rc) return rc;     // what a replay reads
            const rq::Mailbox mb = mailbox_for(dev, true, RQ_POLICY_INPUT_DIM, MbOut::out);
            PolicyCmd cmd;      // what a replay launches: the rows in, in place, the actions out
            cmd.n = batch; cmd.packed = packed_of(pol); cmd.obs = pol->obs; cmd.ld_obs = pol->ld; cmd.hidden = pol->hidden; cmd.ld_h = pol->ld;
            cmd.act = pol->act; cmd.ld_act = pol->ld; cmd.precision = pol->precision; cmd.sas = sas_of(pol, pol->sas_counter, nullptr, 0);
            cmd.mb = mb;
            resident_post(dev, cmd);
            pol->version = fresh_version();                 // as policy_size does for the launch: the hidden state moves on
            rx.policy_streak.n = streak;
            rc = resident_drain(dev); if (rc) return rc;    // (a kernel that had left: noticed in there, replayed as the launch)
            std::memcpy(action, mb.rows_out, (size_t)batch * RQ_ACTION_DIM * sizeof(float));
            return RQ_OK;
        }
    }
    rc = rq::resident_scope_hook(dev); if (rc) return rc;     // a launch on the stream: the resident executor, if any, goes first
    rc = policy_size(pol, batch); if (rc) return rc;
    rx.policy_streak.n = streak;                              // (the two calls above are "something else asked of the device": not this one)
    const bool mailbox = batch < kGpuLayoutMinEnvs && (observation || action);
    if (mailbox) { rc = ensure_mailbox(dev); if (rc) return rc; }
    const bool rows_in = observation && mailbox;      // the kernel reads the mailbox's rows, not d_obs
    if (rows_in) rc = mailbox_put_in(dev, observation, batch, RQ_POLICY_INPUT_DIM, obs_stride);
    else if (observation) rc = host_to_soa(dev, observation, batch, obs_stride, pol->ld, RQ_POLICY_INPUT_DIM, pol->obs);
    if (rc) return rc;
    rq::Mailbox mb{};
    if (mailbox) mb = mailbox_for(dev, rows_in, RQ_POLICY_INPUT_DIM, action ? MbOut::out : MbOut::none);
    rq::ActorStepLaunch a;
    a.n = batch; a.packed = packed_of(pol); a.precision = pol->precision; a.hidden = pol->hidden; a.ld_h = pol->ld; a.mb = mb;
    a.obs = observation ? pol->obs.get() : env->obs.get(); a.ld_obs = observation ? pol->ld : env->ld;
    a.act = action ? pol->act.get() : env->act.get();      a.ld_act = action ? pol->ld : env->ld;
    a.sas = sas_of(pol, pol->sas_counter, nullptr, env ? env->offset : 0);      // (off under a native interval above 1)
    a.interval = pol->native_interval; a.native = pol->rate_counter % pol->native_interval == 0;      // one call counter for the batch
    RQ_HIP_MB(rq::launch_actor_step(dev->stream, a), dev, mb);
    if (rated) pol->rate_counter += 1;
    if (pol->sas_mode == RQ_SAS_SAMPLE) pol->sas_counter += 1;
    if (action && mailbox) return mailbox_copy_out(dev, mb.seq, mb.rows_out, action, (size_t)batch * RQ_ACTION_DIM);
    if (action) return soa_to_host(dev, pol->act, batch, pol->ld, RQ_ACTION_DIM, action);
    return RQ_OK;
}

RQ_API int rq_policy_evaluate_sequence(rq_policy* pol, const float* observation, uint32_t steps, uint32_t batch,
                                uint32_t obs_stride, float* action, int memory) {
    RQ_REQUIRE(pol && observation && action, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(steps > 0 && batch > 0, RQ_ERR_INVALID_ARGUMENT, "empty sequence");
    RQ_REQUIRE(obs_stride >= RQ_POLICY_INPUT_DIM, RQ_ERR_INVALID_ARGUMENT, "obs_stride < 22");
    RQ_REQUIRE(CallMemory::valid(memory), RQ_ERR_INVALID_ARGUMENT, "memory must be 0, 1 or 2");
    RQ_REQUIRE(pol->sas_mode != RQ_SAS_SAMPLE, RQ_ERR_INVALID_ARGUMENT,
               "sequence evaluation is a deterministic pass: RQ_SAS_SAMPLE is defined for evaluate_step and rollouts");
    { const int rate_rc = require_native_rate(pol, "rq_policy_evaluate_sequence"); if (rate_rc) return rate_rc; }
    if (memory != RQ_DST_HOST)      // the kernel moves rows with 8-byte loads and actions with 16-byte stores
        RQ_REQUIRE((reinterpret_cast<uintptr_t>(observation) & 7u) == 0 && (reinterpret_cast<uintptr_t>(action) & 15u) == 0,
                   RQ_ERR_INVALID_ARGUMENT, "device tensors must be 8-byte (observation) / 16-byte (action) aligned");
    rq_device* dev = pol->dev;
    DeviceScope on_device(dev); int rc = on_device.rc; if (rc) return rc;
    rc = policy_size(pol, batch); if (rc) return rc;
    const size_t rows = (size_t)steps * batch;
    CallMemory mem(memory, dev->stream, dev->ordinal);
    if (mem.host()) {
        RQ_HIP(dev->rows.reserve(dev->stream, rows * obs_stride));
        RQ_HIP(dev->rows2.reserve(dev->stream, rows * RQ_ACTION_DIM));
    }
    const float* d_obs = nullptr;          // (the last row ends with its 22 floats: the caller's array need not hold a whole stride there)
    RQ_HIP(mem.in(observation, (rows - 1) * obs_stride + RQ_POLICY_INPUT_DIM, dev->rows.get(), &d_obs));
    float* d_act = mem.out(action, rows * RQ_ACTION_DIM, dev->rows2.get());
    RQ_HIP(rq::launch_actor_sequence(dev->stream, batch, steps, packed_of(pol), d_obs, obs_stride, pol->hidden, pol->ld,
                                     d_act, mode_of(pol)));
    RQ_HIP(mem.finish());
    return RQ_OK;
}

RQ_API int rq_policy_get_hidden(const rq_policy* pol, float* host_out, uint32_t batch) {
    RQ_REQUIRE(pol && host_out, RQ_ERR_INVALID_ARGUMENT, "null argument");
    int rc = policy_size(const_cast<rq_policy*>(pol), batch); if (rc) return rc;
    return soa_to_host(pol->dev, pol->hidden, batch, pol->ld, RQ_POLICY_HIDDEN_DIM, host_out);
}

RQ_API int rq_policy_set_hidden(rq_policy* pol, const float* host_in, uint32_t batch) {
    RQ_REQUIRE(pol && host_in, RQ_ERR_INVALID_ARGUMENT, "null argument");
    DeviceScope on_device(pol->dev); int rc = on_device.rc; if (rc) return rc;
    rc = policy_size(pol, batch); if (rc) return rc;
    return host_to_soa(pol->dev, host_in, batch, RQ_POLICY_HIDDEN_DIM, pol->ld, RQ_POLICY_HIDDEN_DIM, pol->hidden);
}

RQ_API int rq_policy_selftest(rq_policy* pol, const float* input, const float* expected, uint32_t steps, uint32_t batch,
                       float tolerance, float* max_abs_err) {
    RQ_REQUIRE(pol && input && expected, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(steps > 0 && batch > 0, RQ_ERR_INVALID_ARGUMENT, "empty test");
    { const int rate_rc = require_native_rate(pol, "rq_policy_selftest"); if (rate_rc) return rate_rc; }
    // runs on a private policy object so the caller's hidden state is untouched
    rq_policy* tmp = nullptr;
    int rc = policy_mirror(pol); if (rc) return rc;
    rc = policy_images16(pol); if (rc) return rc;
    rc = rq_policy_create(pol->dev, pol->w_host, RQ_POLICY_NUM_WEIGHTS, &tmp); if (rc) return rc;
    tmp->precision = pol->precision;
    tmp->sas_mode = pol->sas_mode == RQ_SAS_SAMPLE ? RQ_SAS_MEAN : pol->sas_mode;   // known answers are deterministic
    if (pol->standardize) {
        tmp->standardize = true;
        std::memcpy(tmp->std_mean, pol->std_mean, sizeof(tmp->std_mean));
        std::memcpy(tmp->std_inv, pol->std_inv, sizeof(tmp->std_inv));
        rc = policy_upload(tmp, tmp->w_host, "rq_policy_selftest");
        if (rc) { rq_policy_destroy(tmp); return rc; }
    }
    std::vector<float> act;
    try { act.resize((size_t)batch * RQ_ACTION_DIM); } catch (const std::bad_alloc&) { rq_policy_destroy(tmp); return fail(RQ_ERR_OUT_OF_MEMORY, "rq_policy_selftest: host allocation failed"); }
    float worst = 0.0f;
    for (uint32_t t = 0; t < steps && rc == RQ_OK; ++t) {
        rc = rq_policy_evaluate_step(tmp, nullptr, input + (size_t)t * batch * RQ_POLICY_INPUT_DIM, batch,
                                     RQ_POLICY_INPUT_DIM, act.data());
        const float* ex = expected + (size_t)t * batch * RQ_ACTION_DIM;
        for (size_t k = 0; k < act.size(); ++k) {
            float d = act[k] - ex[k]; if (d < 0) d = -d;
            if (!(d <= worst)) worst = d;   // NaN-propagating max
        }
    }
    rq_policy_destroy(tmp);
    if (rc) return rc;
    if (max_abs_err) *max_abs_err = worst;
    if (!(worst <= tolerance))
        return fail(RQ_ERR_SELFTEST_FAILED, "rq_policy_selftest: max |out - expected| = " + std::to_string(worst) +
                                                " exceeds tolerance " + std::to_string(tolerance));
    return RQ_OK;
}

}  // extern "C"
