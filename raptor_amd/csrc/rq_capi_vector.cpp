// rq_capi_vector.cpp - the five l2f vector:: functions (README.md:60,61,96,98) and what serves the reference's loop at small batches behind
// them: the pinned mailbox, the observation cache and the speculative policy step (include/raptor_quad.h rq_device_set_speculation);
// rq_step posts to the resident executor (rq_resident.cpp) where it can.  Objects and shared helpers: rq_objects.hpp.
#include "rq_objects.hpp"

namespace rqh {

// ---- small-batch mailbox (below kGpuLayoutMinEnvs envs): rows cross the boundary in pinned host memory
// the kernels read and write themselves, and the host waits on a flag instead of the stream ---------------
constexpr size_t kMailboxRowFloats = (size_t)(kGpuLayoutMinEnvs - 1) * 32;

int ensure_mailbox(rq_device* dev) {
    if (dev->mb_flag) return RQ_OK;
    void *flag = nullptr, *in = nullptr, *out = nullptr;
    RQ_HIP(hipHostMalloc(&flag, 64, hipHostMallocDefault));
    *static_cast<volatile uint32_t*>(flag) = 0;
    hipError_t e1 = hipHostMalloc(&in, kMailboxRowFloats * sizeof(float), hipHostMallocDefault);
    hipError_t e2 = hipHostMalloc(&out, kMailboxRowFloats * sizeof(float), hipHostMallocDefault);
    void* obs = nullptr;
    hipError_t e3 = hipMalloc(&dev->mb_counter, sizeof(uint32_t));
    if (e3 == hipSuccess) e3 = hipMemsetAsync(dev->mb_counter, 0, sizeof(uint32_t), dev->stream);
    if (e3 == hipSuccess) e3 = hipHostMalloc(&obs, kMailboxRowFloats * sizeof(float), hipHostMallocDefault);
    void* actrows = nullptr;
    if (e3 == hipSuccess) e3 = hipHostMalloc(&actrows, (size_t)kGpuLayoutMinEnvs * RQ_ACTION_DIM * sizeof(float), hipHostMallocDefault);
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) {
        (void)hipHostFree(flag); if (in) (void)hipHostFree(in); if (out) (void)hipHostFree(out);
        if (obs) (void)hipHostFree(obs);
        if (actrows) (void)hipHostFree(actrows);
        if (dev->mb_counter) { (void)hipFree(dev->mb_counter); dev->mb_counter = nullptr; }
        return fail(RQ_ERR_OUT_OF_MEMORY, "ensure_mailbox: pinned host allocation failed");
    }
    dev->mb_flag = static_cast<uint32_t*>(flag);
    dev->mb_in = static_cast<float*>(in);
    dev->mb_out = static_cast<float*>(out);
    dev->mb_obs = static_cast<float*>(obs);
    dev->mb_act = static_cast<float*>(actrows);
    return RQ_OK;
}

// a speculated policy step that was launched is about to be superseded or was passed over: count it
void speculation_unused(rq_device* dev) {
    if (!dev->sp_outstanding) return;
    dev->sp_outstanding = false;
    if (++dev->sp_misses >= kSpeculationMissLimit) dev->sp_suspended = true;
}

// ---- observation cache (rq_device::oc_*) ------------------------------------------------------------------
void obs_cache_drop(rq_device* dev) { dev->oc_env = nullptr; dev->oc_state[0] = dev->oc_state[1] = nullptr; }

bool obs_cache_holds(const rq_device* dev, const rq_env* env, const rq_params* params, const rq_state* state) {
    if (dev->oc_env != env || dev->oc_env_uid != env->uid || env->obs_exposed || dev->oc_params != params || params->exposed || params->version != dev->oc_params_version ||
        state->exposed)
        return false;
    for (int k = 0; k < 2; ++k)
        if (dev->oc_state[k] == state && dev->oc_version[k] == state->version) return true;
    return false;
}

// spin until the launch with sequence number seq (or a later one: launches finish in stream order) signalled.  While the
// resident executor runs, the work waited for may be a command posted to it: if it has left (`exited`) without consuming the
// command, resident_gone() replays the command as launches on the stream and the wait goes on.
int mailbox_wait(rq_device* dev, uint32_t seq) {
    const ResidentExecutor& rx = dev->resident;
    for (uint64_t spins = 1;; ++spins) {
        const uint32_t f = __atomic_load_n(dev->mb_flag, __ATOMIC_ACQUIRE);
        if ((int32_t)(f - seq) >= 0) return RQ_OK;
        if (rx.running && (spins & 0xFFu) == 0 && resident_left(dev)) {
            const int rc = resident_gone(dev); if (rc) return rc;
            continue;
        }
        if ((spins & 0xFFFFu) == 0) {           // every ~100 us: is the stream still alive?
            const hipError_t q = hipStreamQuery(rx.running ? rx.stream : dev->stream);
            if (q == hipSuccess) {
                if (rx.running) { const int rc = resident_gone(dev); if (rc) return rc; continue; }
                const uint32_t g = __atomic_load_n(dev->mb_flag, __ATOMIC_ACQUIRE);
                if ((int32_t)(g - seq) >= 0) return RQ_OK;
                return fail(RQ_ERR_HIP, "mailbox_wait: the stream drained without the kernel signalling");
            }
            if (q != hipErrorNotReady) RQ_HIP(q);
        }
        __builtin_ia32_pause();
    }
}

// before the host overwrites mb_in: the last launch reading it must have finished
int mailbox_in_free(rq_device* dev) {
    if (dev->mb_in_busy == 0) return RQ_OK;
    const int rc = mailbox_wait(dev, dev->mb_in_busy);
    if (rc == RQ_OK) dev->mb_in_busy = 0;
    return rc;
}

rq::Mailbox mailbox_for(rq_device* dev, const float* rows_in, uint32_t in_stride, float* rows_out) {
    rq::Mailbox mb{};
    mb.rows_in = rows_in; mb.in_stride = in_stride; mb.rows_out = rows_out;
    mb.counter = dev->mb_counter; mb.flag = dev->mb_flag;
    if (++dev->mb_seq == 0) ++dev->mb_seq;      // 0 means "nothing pending"
    mb.seq = dev->mb_seq;
    if (rows_in) dev->mb_in_busy = mb.seq;
    return mb;
}

// a launch that was handed a mailbox failed: nothing will ever publish its sequence number
void mailbox_abort(rq_device* dev, const rq::Mailbox& mb) {
    if (mb.flag == nullptr) return;
    if (dev->mb_in_busy == mb.seq) dev->mb_in_busy = 0;
    if (dev->mb_seq == mb.seq) dev->mb_seq = mb.seq - 1;      // 0 ("nothing pending") is skipped by mailbox_for
}

// the two launches of a small-batch step on the device's stream (what rounds 3-5 always did; now also the replay of a command the
// resident executor never consumed)
hipError_t launch_step_pair(rq_device* dev, const StepPair& p) {
    hipError_t e = rq::launch_step(dev->stream, p.b, p.c, p.params, p.state_in, p.act, p.state_out, p.st, /*rollout=*/0, 0u, p.sc, p.seed,
                                   nullptr, nullptr, p.mb_step, p.obs_alt, rq::NoiseCfg{}, false, 0u, nullptr);
    if (e == hipSuccess && p.spec)
        e = rq::launch_actor_step(dev->stream, p.b.n, p.packed, p.obs_alt, p.b.ld, p.hidden_out, p.ld_h, p.pol_act, p.ld_h, nullptr,
                                  p.precision, p.sas, p.mb_spec, p.hidden_in);
    return e;
}


}  // namespace rqh

using namespace rqh;

extern "C" {

RQ_API int rq_device_set_speculation(rq_device* dev, int enable) {
    RQ_REQUIRE(dev, RQ_ERR_INVALID_ARGUMENT, "null argument");
    dev->speculate = enable != 0;
    dev->sp_suspended = false; dev->sp_misses = 0;
    if (!dev->speculate) { dev->sp_policy = nullptr; dev->sp_outstanding = false; }
    return RQ_OK;
}

RQ_API int rq_device_get_speculation(const rq_device* dev, int* enabled, int* suspended, uint32_t* consecutive_misses) {
    RQ_REQUIRE(dev, RQ_ERR_INVALID_ARGUMENT, "null argument");
    if (enabled) *enabled = dev->speculate ? 1 : 0;
    if (suspended) *suspended = dev->sp_suspended ? 1 : 0;
    if (consecutive_misses) *consecutive_misses = dev->sp_misses;
    return RQ_OK;
}

// ---------------------------------------------------------------------------- l2f vector::
RQ_API int rq_sample_initial_parameters(rq_device* dev, rq_env* env, rq_params* params, rq_rng* rng) {
    int rc = check_env_objects(dev, env, params, nullptr); if (rc) return rc;
    RQ_REQUIRE(params && rng, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(rng->initialized, RQ_ERR_NOT_INITIALIZED, "initialize_rng was not called");
    DeviceScope on_device(dev); rc = on_device.rc; if (rc) return rc;
    RQ_HIP(rq::launch_sample_params(dev->stream, batch_of(env), rq::sample_cfg(env->cfg), rng->seed,
                                    rng->param_epoch, params->d));
    params->version = fresh_version();
    rng->param_epoch += 1;
    return RQ_OK;
}

RQ_API int rq_sample_initial_state(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state, rq_rng* rng) {
    int rc = check_env_objects(dev, env, params, state); if (rc) return rc;
    RQ_REQUIRE(params && state && rng, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(rng->initialized, RQ_ERR_NOT_INITIALIZED, "initialize_rng was not called");
    DeviceScope on_device(dev); rc = on_device.rc; if (rc) return rc;
    rc = state_make_private(state, false); if (rc) return rc;
    RQ_HIP(rq::launch_sample_state(dev->stream, batch_of(env), rq::sample_cfg(env->cfg), rng->seed, params->d,
                                   state->d, env->st));
    state->version = fresh_version();
    return RQ_OK;
}

RQ_API int rq_observe(rq_device* dev, rq_env* env, const rq_params* params, const rq_state* state, float* observation,
               rq_rng* rng) {
    int rc = check_env_objects(dev, env, params, state); if (rc) return rc;
    RQ_REQUIRE(params && state && rng, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(rng->initialized, RQ_ERR_NOT_INITIALIZED, "initialize_rng was not called");
    DeviceScope on_device(dev, rq::KeepResident{}); rc = on_device.rc; if (rc) return rc;
    if (env->n < kGpuLayoutMinEnvs && !rq::noise_enabled(env->cfg) && obs_cache_holds(dev, env, params, state)) {
        // the step that produced this state assembled its observation already: obs_alt holds it on the device (swapped
        // in here), the pinned rows hold it for the host - wait for that launch's flag (usually long set) and copy; no launch
        rng->epoch += 1;
        if (dev->oc_in_alt) { std::swap(env->obs, env->obs_alt); dev->oc_in_alt = false; }
        if (!observation) return RQ_OK;
        rc = mailbox_wait(dev, dev->oc_seq); if (rc) return rc;
        std::memcpy(observation, dev->mb_obs, (size_t)env->n * RQ_OBSERVATION_DIM * sizeof(float));
        return RQ_OK;
    }
    rc = rq::resident_scope_hook(dev); if (rc) return rc;     // a launch on the stream: the resident executor, if any, goes first
    if (dev->oc_env == env) obs_cache_drop(dev);       // a real observation replaces whatever was cached
    const bool mailbox = observation && env->n < kGpuLayoutMinEnvs;
    rq::Mailbox mb{};
    if (mailbox) { rc = ensure_mailbox(dev); if (rc) return rc; mb = mailbox_for(dev, nullptr, 0, dev->mb_out); }
    RQ_HIP_MB(rq::launch_observe(dev->stream, batch_of(env), rq::noise_cfg(env->cfg), rq::noise_enabled(env->cfg),
                                 rng->seed, rng->epoch, nullptr, params->d, state->d, env->obs, mb), dev, mb);
    rng->epoch += 1;
    if (mailbox) {
        rc = mailbox_wait(dev, mb.seq); if (rc) return rc;
        std::memcpy(observation, dev->mb_out, (size_t)env->n * RQ_OBSERVATION_DIM * sizeof(float));
        return RQ_OK;
    }
    if (observation) return soa_to_host(dev, env->obs, env->n, env->ld, RQ_OBSERVATION_DIM, observation);
    return RQ_OK;
}

RQ_API int rq_step(rq_device* dev, rq_env* env, const rq_params* params, const rq_state* state, const float* action,
            rq_state* next_state, rq_rng* rng, float* dts) {
    int rc = check_env_objects(dev, env, params, state); if (rc) return rc;
    RQ_REQUIRE(params && state && next_state && rng, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(next_state->env == env, RQ_ERR_SHAPE_MISMATCH, "next_state belongs to another env");
    DeviceScope on_device(dev, rq::KeepResident{}); rc = on_device.rc; if (rc) return rc;
    // small batches: the kernel also assembles the observation of the state it writes (device buffer + pinned rows):
    // the observe() of the next loop iteration then needs no launch (obs_cache_holds)
    const bool cache_obs = env->n < kGpuLayoutMinEnvs && !rq::noise_enabled(env->cfg) && !params->exposed &&
                           !next_state->exposed && !env->obs_exposed;
    if (cache_obs) speculation_unused(dev);      // the previous step's speculated policy step, if nobody took it (this may suspend speculation)
    // the policy a speculative step would evaluate on that observation (see rq_device::sp_*)
    rq_policy* pol = cache_obs && dev->speculate && !dev->sp_suspended && action ? dev->last_policy : nullptr;
    if (pol && !(policy_registry(pol, 0) && pol->dev == dev && pol->batch == env->n && pol->ld == env->ld && pol->hidden &&
                 pol->hidden_alt && !pol->needs_reset && pol->sas_mode != RQ_SAS_SAMPLE))
        pol = nullptr;
    // Could the resident executor take this step?  The loop's own shape only: host actions in, observation cached, a speculated
    // fp32 policy step behind it, out of place, on buffers the library alone writes - and the same objects as the kernel in flight.
    ResidentExecutor& rx = dev->resident;
    const bool eligible = rx.enabled && pol && env->obs_alt && env->n <= kResidentMaxEnvs && next_state != state && !state->exposed &&
                          pol->precision == RQ_POLICY_FP32 && pol->sas_mode == RQ_SAS_OFF;
    const uint64_t now_ns = eligible ? host_now_ns() : 0;
    // in a row = the same env: two loops taking turns keep their launches
    const uint32_t streak = rx.loop_streak.n = rx.loop_streak.follow(eligible, now_ns, nullptr, env->uid);
    rx.policy_streak.n = 0;
    ResidentBinding want{};
    if (eligible)
        want = {false, env, env->uid, params, params->version, pol, packed_of(pol), env->n, env->cfg, rng->seed, {env->obs, env->obs_alt},
                {pol->hidden, pol->hidden_alt}};
    bool resident = false;
    rc = resident_admit(dev, eligible, want, now_ns, streak, &resident); if (rc) return rc;
    // next_state is written in full: if it shares its buffer (state.assign(next_state) of the previous iteration) it
    // gets another one; stepping a state in place (next_state == state) keeps the contents it is about to read
    rc = state_make_private(next_state, next_state == state); if (rc) return rc;
    if (cache_obs && !env->obs_alt) {
        RQ_HIP(hipMalloc(&env->obs_alt, (size_t)RQ_OBSERVATION_DIM * env->ld * sizeof(float)));
        RQ_HIP(hipMemsetAsync(env->obs_alt, 0, (size_t)RQ_OBSERVATION_DIM * env->ld * sizeof(float), dev->stream));
    }
    rq::Mailbox mb{};
    if (env->n < kGpuLayoutMinEnvs && (action || cache_obs)) {
        // the kernel reads the actions from the mailbox (and files them in env->act); nothing to wait for
        rc = ensure_mailbox(dev); if (rc) return rc;
        if (action) {
            rc = mailbox_in_free(dev); if (rc) return rc;
            std::memcpy(dev->mb_in, action, (size_t)env->n * RQ_ACTION_DIM * sizeof(float));
        }
        if (cache_obs && dev->oc_env) {                // the pinned rows are about to be rewritten: a host reader of the
            rc = mailbox_wait(dev, dev->oc_seq); if (rc) return rc;     // previous ones cannot exist (calls are synchronous),
        }                                              // but their producer must be done before the next one starts
        mb = mailbox_for(dev, action ? dev->mb_in : nullptr, RQ_ACTION_DIM, cache_obs ? dev->mb_obs : nullptr);
    } else if (action) {
        rc = host_to_soa(dev, action, env->n, RQ_ACTION_DIM, env->ld, RQ_ACTION_DIM, env->act);
        if (rc) return rc;
    }
    obs_cache_drop(dev);
    next_state->version = fresh_version();
    StepPair pair{};
    pair.b = batch_of(env); pair.c = rq::step_cfg(env->cfg); pair.sc = rq::sample_cfg(env->cfg); pair.seed = rng->seed;
    pair.params = params->d; pair.state_in = state->d; pair.act = env->act; pair.state_out = next_state->d; pair.st = env->st;
    pair.mb_step = mb; pair.obs_alt = cache_obs ? env->obs_alt : nullptr;
    pair.spec = pol != nullptr;
    if (pol) {
        pair.packed = packed_of(pol); pair.hidden_out = pol->hidden_alt; pair.ld_h = pol->ld; pair.pol_act = pol->act;
        pair.precision = pol->precision; pair.sas = sas_of(pol, 0, nullptr, 0); pair.hidden_in = pol->hidden;
        pair.mb_spec = mailbox_for(dev, nullptr, 0, dev->mb_act);
    }
    bool posted = false;
    if (resident) {
        if (!rx.running) {
            rq::ResidentArgs ra{};
            ra.b = pair.b; ra.c = pair.c; ra.sc = pair.sc; ra.seed = pair.seed;
            ra.params = pair.params; ra.act = pair.act; ra.st = pair.st;
            ra.ld_h = pol->ld; ra.pol_act = pol->act;
            ra.rows_action = dev->mb_in; ra.rows_obs = dev->mb_obs; ra.rows_act = dev->mb_act; ra.flag = dev->mb_flag;
            rc = resident_start(dev, ra, want);
        }
        if (rc == RQ_OK && rx.running) rc = resident_drain(dev);     // one command slot: the previous command must have been taken out of it
        if (rc) { mailbox_abort(dev, pair.mb_spec); mailbox_abort(dev, mb); return rc; }
        if (rx.running) {
            uint32_t sum = 0;
            const uint32_t* au = reinterpret_cast<const uint32_t*>(dev->mb_in);
            for (uint32_t k = 0; k < env->n * RQ_ACTION_DIM; ++k) sum += au[k];
            if (env->n <= rq::kResidentSmallEnvs || rx.cmd_on_device) {     // the small kernel reads the rows in the same load as the
                __m128i* rows = reinterpret_cast<__m128i*>(resident_rows(dev));   // command line; in device memory every kernel reads them there
                for (uint32_t k = 0; k < env->n; ++k) _mm_store_si128(rows + k, _mm_loadu_si128(reinterpret_cast<const __m128i*>(au) + k));
            }
            resident_post(dev, pair, sum);
            posted = true;
        }
    }
    if (!posted) {
        const hipError_t e = launch_step_pair(dev, pair);
        if (e != hipSuccess) {
            if (pair.spec) mailbox_abort(dev, pair.mb_spec);
            mailbox_abort(dev, mb);
            return fail(RQ_ERR_HIP, std::string("rq_step: launch -> ") + hipGetErrorString(e));
        }
    }
    if (cache_obs) {
        dev->oc_env = env; dev->oc_env_uid = env->uid; dev->oc_params = params; dev->oc_params_version = params->version;
        dev->oc_state[0] = next_state; dev->oc_version[0] = next_state->version;
        dev->oc_state[1] = nullptr;
        dev->oc_seq = mb.seq; dev->oc_n = env->n;
        dev->oc_in_alt = true;
        dev->sp_policy = nullptr;
        if (pol) {
            dev->sp_policy = pol; dev->sp_policy_version = pol->version; dev->sp_batch = env->n;
            dev->sp_seq = pair.mb_spec.seq; dev->sp_oc_seq = dev->oc_seq;
            dev->sp_outstanding = true;
        }
    }
    if (dts) for (uint32_t i = 0; i < env->n; ++i) dts[i] = env->cfg.dt;
    return RQ_OK;
}

RQ_API int rq_env_observation_device_ptr(const rq_env* env, float** p) {
    RQ_REQUIRE(env && p, RQ_ERR_INVALID_ARGUMENT, "null argument");
    const_cast<rq_env*>(env)->obs_exposed = true;
    *p = env->obs; return RQ_OK;
}
RQ_API int rq_env_action_device_ptr(const rq_env* env, float** p) {
    RQ_REQUIRE(env && p, RQ_ERR_INVALID_ARGUMENT, "null argument");
    *p = env->act; return RQ_OK;
}
RQ_API int rq_env_get_observation(const rq_env* env, float* host_out) {
    RQ_REQUIRE(env && host_out, RQ_ERR_INVALID_ARGUMENT, "null argument");
    return soa_to_host(env->dev, env->obs, env->n, env->ld, RQ_OBSERVATION_DIM, host_out);
}
RQ_API int rq_env_get_action(const rq_env* env, float* host_out) {
    RQ_REQUIRE(env && host_out, RQ_ERR_INVALID_ARGUMENT, "null argument");
    return soa_to_host(env->dev, env->act, env->n, env->ld, RQ_ACTION_DIM, host_out);
}
RQ_API int rq_env_set_action(rq_env* env, const float* host_in) {
    RQ_REQUIRE(env && host_in, RQ_ERR_INVALID_ARGUMENT, "null argument");
    return host_to_soa(env->dev, host_in, env->n, RQ_ACTION_DIM, env->ld, RQ_ACTION_DIM, env->act);
}

}  // extern "C"
