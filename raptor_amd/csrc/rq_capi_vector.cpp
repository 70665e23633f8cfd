// rq_capi_vector.cpp - the five l2f vector:: functions (README.md:60,61,96,98); small batches go through rq_small_batch.cpp, and rq_step
// posts to the resident executor (rq_resident.cpp) where it can.  Objects and shared helpers: rq_objects.hpp.
#include "rq_objects.hpp"

using namespace rqh;

extern "C" {

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
    // a sensor schedule: what is observed depends on the env's readings, not on (params, state) alone - no cache, as with noise; and
    // k_sensor_apply delivers behind k_observe, so the rows leave through soa_to_host, not through the mailbox k_observe fills
    const bool sensor = env->has_sensor_schedule();
    if (env->n < kGpuLayoutMinEnvs && !rq::noise_enabled(env->cfg) && !sensor && obs_cache_holds(dev, env, params, state)) {
        rng->epoch += 1;
        return obs_cache_read(dev, env, observation);
    }
    rc = rq::resident_scope_hook(dev); if (rc) return rc;     // a launch on the stream: the resident executor, if any, goes first
    obs_cache_drop_if(dev, env);
    const bool mailbox = observation && env->n < kGpuLayoutMinEnvs && !sensor;
    rq::Mailbox mb{};
    if (mailbox) { rc = ensure_mailbox(dev); if (rc) return rc; mb = mailbox_for(dev, false, 0, MbOut::out); }
    RQ_HIP_MB(rq::launch_observe(dev->stream, batch_of(env), rq::noise_cfg(env->cfg), rq::noise_enabled(env->cfg),
                                 rng->seed, rng->epoch, nullptr, params->d, state->d, env->obs, mb), dev, mb);
    if (sensor) {
        const auto& slot = env->schedule[kSensor];
        const rq::SensorPtrs sn{static_cast<const rq_sensor_bank*>(slot.bank)->steps.get(), slot.row0, env->sensor_history.ring, slot.bank->rows, 0u};
        RQ_HIP(rq::launch_sensor_apply(dev->stream, batch_of(env), env->st, env->obs, sn));
    }
    rng->epoch += 1;
    if (mailbox) return mailbox_copy_out(dev, mb.seq, mb.rows_out, observation, (size_t)env->n * RQ_OBSERVATION_DIM);
    if (observation) return soa_to_host(dev, env->obs, env->n, env->ld, RQ_OBSERVATION_DIM, observation);
    return RQ_OK;
}

RQ_API int rq_step(rq_device* dev, rq_env* env, const rq_params* params, const rq_state* state, const float* action,
            rq_state* next_state, rq_rng* rng, float* dts) {
    int rc = check_env_objects(dev, env, params, state); if (rc) return rc;
    RQ_REQUIRE(params && state && next_state && rng, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(next_state->env == env, RQ_ERR_SHAPE_MISMATCH, "next_state belongs to another env");
    SchedulePtrs sched[kScheduleKinds];
    rc = env_schedules(__func__, env, sched); if (rc) return rc;  // the env's schedules, refused before anything is enqueued
    DeviceScope on_device(dev, rq::KeepResident{}); rc = on_device.rc; if (rc) return rc;
    // small batches: the kernel also assembles the observation of the state it writes, for the next observe() (ObservationCache)
    // (nor while a sensor schedule is attached: rq_observe then delivers out of the env's readings, with plain launches)
    const bool cache_obs = env->n < kGpuLayoutMinEnvs && !rq::noise_enabled(env->cfg) && !params->exposed &&
                           !next_state->exposed && !env->obs_exposed && !env->has_sensor_schedule();
    rq_policy* pol = speculation_candidate(dev, env, cache_obs, action != nullptr);     // evaluated on that observation, speculatively
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
        RQ_HIP(env->obs_alt.alloc((size_t)RQ_OBSERVATION_DIM * env->ld));
        RQ_HIP(hipMemsetAsync(env->obs_alt, 0, (size_t)RQ_OBSERVATION_DIM * env->ld * sizeof(float), dev->stream));
    }
    rq::Mailbox mb{};
    if (env->n < kGpuLayoutMinEnvs && (action || cache_obs)) rc = mailbox_for_step(dev, action, env->n, cache_obs, &mb);
    else if (action) rc = host_to_soa(dev, action, env->n, RQ_ACTION_DIM, env->ld, RQ_ACTION_DIM, env->act);
    if (rc) return rc;
    obs_cache_drop(dev);
    next_state->version = fresh_version();
    StepPair pair{};
    rq::EnvStepLaunch& es = pair.step;
    es.b = batch_of(env); es.c = rq::step_cfg(env->cfg); es.sc = rq::sample_cfg(env->cfg); es.seed = rng->seed;
    es.params = params->d; es.state = state->d; es.action = env->act; es.next_state = next_state->d; es.st = env->st;
    es.mb = mb; es.obs_of_next = cache_obs ? env->obs_alt.get() : nullptr; set_schedules(es, sched);
    pair.spec = pol != nullptr;
    if (pol) {      // on the observation the step leaves, out of place: hidden -> hidden_alt
        rq::ActorStepLaunch& as = pair.actor;
        as.n = env->n; as.packed = packed_of(pol); as.obs = es.obs_of_next; as.ld_obs = env->ld;
        as.hidden_in = pol->hidden; as.hidden = pol->hidden_alt; as.ld_h = pol->ld; as.act = pol->act; as.ld_act = pol->ld;
        as.precision = pol->precision; as.sas = sas_of(pol, 0, nullptr, 0);
        as.mb = mailbox_for(dev, false, 0, MbOut::act);
    }
    if (resident) {
        if (!rx.running) {
            rq::ResidentArgs ra{};
            ra.b = es.b; ra.c = es.c; ra.sc = es.sc; ra.seed = es.seed;
            ra.params = es.params; ra.act = es.action; ra.st = es.st; ra.ld_h = pol->ld; ra.pol_act = pol->act;
            rc = resident_start(dev, ra, want);
        }
        if (rc == RQ_OK && rx.running) rc = resident_drain(dev);     // one command slot: the previous command must have been taken out of it
        if (rc) { mailbox_abort(dev, pair.actor.mb); mailbox_abort(dev, mb); return rc; }
    }
    if (resident && rx.running) {
        resident_post(dev, pair);
    } else {
        const hipError_t e = launch_step_pair(dev, pair);
        if (e != hipSuccess) {
            mailbox_abort(dev, pair.actor.mb); mailbox_abort(dev, mb);      // (pair.actor.mb is empty without a speculated step)
            return fail(RQ_ERR_HIP, std::string("rq_step: launch -> ") + hipGetErrorString(e));
        }
    }
    if (cache_obs) obs_cache_fill(dev, env, params, next_state, mb.seq, pol, pair.actor.mb.seq);
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
