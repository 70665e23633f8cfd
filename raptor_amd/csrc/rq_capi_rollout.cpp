// rq_capi_rollout.cpp - the loop body README.md:95-99 x K on the device (fused kernel, or the chained kernels under a hipGraph built node
// by node), the trajectory buffer and relabelling a recorded trajectory with a policy.
#include "rq_objects.hpp"

#include <cmath>

namespace rqh {

int traj_block_to_host(rq_device* dev, const float* d_soa, uint32_t steps, uint32_t n, uint32_t ld, uint32_t dim,
                              float* host) {
    const size_t per_step = (size_t)n * dim * sizeof(float);
    uint32_t chunk = (uint32_t)std::min<size_t>(steps, std::max<size_t>(1, ((size_t)1 << 30) / per_step));   // <= 1 GiB scratch
    if (chunk > 65535u) chunk = 65535u;
    RQ_HIP(dev->rows.reserve(dev->stream, (size_t)n * dim * chunk));
    for (uint32_t s0 = 0; s0 < steps; s0 += chunk) {
        const uint32_t c = std::min(chunk, steps - s0);
        RQ_HIP(rq::launch_soa_to_rows(dev->stream, d_soa + (size_t)s0 * dim * ld, ld, dim, n, dev->rows, c));
        RQ_HIP(hipMemcpyAsync(host + (size_t)s0 * n * dim, dev->rows, per_step * c, hipMemcpyDeviceToHost, dev->stream));
        RQ_HIP(hipStreamSynchronize(dev->stream));
    }
    return RQ_OK;
}

// `actor`: the caller was given what acts (a policy; a bank and its assignment)
int rollout_check(RolloutFrame& f, const rq_device* dev, const rq_env* env, const rq_params* params, const rq_state* state, const rq_rng* rng,
                  bool actor, uint32_t n_steps, int mode, uint32_t flags, const rq_trajectory* traj) {
    int rc = check_env_objects(dev, env, params, state); if (rc) return rc;
    RQ_REQUIRE(params && state && actor && rng, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(rng->initialized, RQ_ERR_NOT_INITIALIZED, "initialize_rng was not called");
    RQ_REQUIRE(mode == RQ_ROLLOUT_FUSED || mode == RQ_ROLLOUT_CHAINED, RQ_ERR_INVALID_ARGUMENT, "unknown mode");
    RQ_REQUIRE((flags & ~(uint32_t)RQ_ROLLOUT_AUTORESET) == 0, RQ_ERR_INVALID_ARGUMENT, "unknown flags");
    if (traj) {
        RQ_REQUIRE(traj->env == env, RQ_ERR_SHAPE_MISMATCH, "trajectory belongs to another env");
        RQ_REQUIRE((uint64_t)traj->length + n_steps <= traj->capacity, RQ_ERR_INVALID_ARGUMENT,
                   "trajectory buffer too small for this rollout");
        f.tp = {traj->obs, traj->act, traj->rew, traj->done, traj->length};
    }
    return env_wrench("rollout", env, &f.wr);
}

int env_wrench(const char* who, const rq_env* env, rq::WrenchPtrs* wr) {
    *wr = rq::WrenchPtrs{};
    const rq_wrench_bank* bank = env->wrench;
    if (!bank) return RQ_OK;
    if (bank->rows < env->cfg.episode_step_limit)
        return fail(RQ_ERR_INVALID_ARGUMENT, std::string(who) + ": the env's wrench schedule has fewer rows (" + std::to_string(bank->rows) +
                                                 ") than episode_step_limit (" + std::to_string(env->cfg.episode_step_limit) +
                                                 "): every table must cover an episode");
    *wr = {bank->d, env->wrench_row0, bank->rows, bank->units == RQ_WRENCH_RELATIVE ? 1u : 0u};
    return RQ_OK;
}

int wrench_refuses_fused(const char* who, const char* what) {
    return fail(RQ_ERR_INVALID_ARGUMENT, std::string(who) + ": the env carries a wrench schedule, which the fused kernel of " + what +
                                             " is not taught: fly it with mode RQ_ROLLOUT_CHAINED (\"chained\"), or detach the schedule");
}

int rollout_check_reference(const char* who, const rq_device* dev, const rq_env* env, const rq_reference* ref) {
    if (ref->dev != dev) return fail(RQ_ERR_SHAPE_MISMATCH, std::string(who) + ": reference lives on another device");
    if (ref->rows < env->cfg.episode_step_limit)
        return fail(RQ_ERR_INVALID_ARGUMENT,
                    std::string(who) + ": reference has fewer rows than episode_step_limit: the table must cover an episode");
    return RQ_OK;
}

int rollout_track(RolloutFrame& f, rq_env* env, const rq_reference* ref) {
    if (!ref) return RQ_OK;
    const int rc = env_track_stats(env, &f.trk.sq, &f.trk.steps); if (rc) return rc;
    f.trk.ref = ref->d; f.trk.rows = ref->rows;
    return RQ_OK;
}

int rollout_check_reference_bank(const char* who, const rq_device* dev, const rq_env* env, const rq_reference_bank* refs,
                                 const uint32_t* reference_id) {
    if (!refs) return RQ_OK;
    if (refs->dev != dev) return fail(RQ_ERR_SHAPE_MISMATCH, std::string(who) + ": reference bank lives on another device");
    if (refs->rows < env->cfg.episode_step_limit)
        return fail(RQ_ERR_INVALID_ARGUMENT,
                    std::string(who) + ": reference bank has fewer rows than episode_step_limit: every table must cover an episode");
    for (uint32_t i = 0; i < env->n; ++i)
        if (reference_id[i] >= refs->n_refs)
            return fail(RQ_ERR_INVALID_ARGUMENT, std::string(who) + ": reference id out of range: env " + std::to_string(i) +
                                                     " names reference " + std::to_string(reference_id[i]) + " of a bank of " +
                                                     std::to_string(refs->n_refs));
    return RQ_OK;
}

int rollout_track_refs(RolloutFrame& f, rq_device* dev, rq_env* env, const rq_reference_bank* refs, const uint32_t* reference_id) {
    if (!refs) return RQ_OK;
    const uint32_t n = env->n;
    int rc = env_track_stats(env, &f.trk.sq, &f.trk.steps); if (rc) return rc;
    uint32_t* row0 = f.trk.steps + env->ld;                       // the block's third array
    const bool same = env->row0_valid && env->row0_key == refs->uid && env->row0_ids.size() == n &&
                      std::memcmp(env->row0_ids.data(), reference_id, (size_t)n * sizeof(uint32_t)) == 0;
    if (!same) {
        env->row0_valid = false;
        std::vector<uint32_t> first;
        try {                                   // nothing throws across the boundary
            env->row0_ids.assign(reference_id, reference_id + n);
            first.resize(n);
        } catch (const std::bad_alloc&) {
            return fail(RQ_ERR_OUT_OF_MEMORY, "reference bank: host allocation failed");
        }
        for (uint32_t i = 0; i < n; ++i) first[i] = reference_id[i] * refs->rows;       // < n_refs * rows < 2^28
        RQ_HIP(hipStreamSynchronize(dev->stream));                // a rollout in flight reads the rows of the ids before
        RQ_HIP(hipMemcpyAsync(row0, first.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, dev->stream));
        RQ_HIP(hipStreamSynchronize(dev->stream));                // `first` is pageable and goes away
        env->row0_valid = true;
        env->row0_key = refs->uid;
        env->row0_gen = fresh_version();
    }
    f.trk.ref = refs->d; f.trk.rows = refs->rows; f.trk.row0_at = env->ld; f.row0_gen = env->row0_gen;
    return RQ_OK;
}

int rollout_begin(RolloutFrame& f, rq_device* dev, rq_env* env, rq_state* state, uint32_t n_steps, uint32_t flags, rq_trajectory* traj) {
    obs_cache_drop_if(dev, env);
    if (n_steps) { const int rc = state_make_private(state, true); if (rc) return rc; }      // steps the state in place
    f.b = batch_of(env);
    f.sc = rq::step_cfg(env->cfg);
    f.nc = rq::noise_cfg(env->cfg);
    f.smp = rq::sample_cfg(env->cfg);
    f.noise = rq::noise_enabled(env->cfg);
    if (traj && n_steps && !(flags & RQ_ROLLOUT_AUTORESET))   // steps a frozen wave never reaches read as "not stepped"
        RQ_HIP(hipMemsetAsync(traj->done + (size_t)traj->length * env->ld, 4, (size_t)n_steps * env->ld, dev->stream));
    return RQ_OK;
}

void rollout_end(rq_state* state, rq_rng* rng, uint32_t n_steps, rq_trajectory* traj) {
    rng->epoch += n_steps;
    if (traj) traj->length += n_steps;
    if (n_steps) state->version = fresh_version();
}

rq::FusedArgs fused_args(const RolloutFrame& f, const rq_env* env, const rq_params* params, const rq_state* state, const rq_rng* rng,
                         uint32_t n_steps, uint32_t flags, unsigned long long* span) {
    rq::FusedArgs a;
    a.b = f.b; a.c = f.sc; a.nc = f.nc; a.sc = f.smp; a.noise = f.noise;
    a.seed = rng->seed; a.epoch0 = rng->epoch; a.n_steps = n_steps;
    a.autoreset = (flags & RQ_ROLLOUT_AUTORESET) != 0;
    a.params = params->d; a.state = state->d; a.st = env->st;
    a.traj = f.tp; a.trk = f.trk; a.wr = f.wr; a.span = span;
    return a;
}

int fused_span_begin(const char* who, rq_device* dev, const rq_env* env, uint32_t n_steps, unsigned long long** span) {
    if (dev->k_timing && n_steps) {                   // one (in, out) record per wave = per workgroup of the fused kernel
        const uint32_t waves = (env->n + 63u) / 64u;
        const hipError_t e = dev->k_span.reserve(dev->stream, (size_t)waves * 5);
        if (e != hipSuccess) return hip_failed(who, "dev->k_span.reserve(dev->stream, (size_t)waves * 5)", e);
        dev->k_span_used = waves;
    }
    *span = dev->k_timing ? dev->k_span.get() : nullptr;
    return RQ_OK;
}

void fused_span_end(rq_device* dev, uint32_t n_steps) {
    dev->k_timed = dev->k_timing && n_steps > 0;
    dev->k_fetched = false;
}

}  // namespace rqh

using namespace rqh;

extern "C" {

// ---------------------------------------------------------------------------- Rollout ---
static constexpr uint32_t kGraphSteps = 25;   // steps per captured graph (divides the 500-step episode)
static constexpr size_t kMaxGraphs = 8;       // executable graphs kept per env (one per distinct argument set)

static int rollout_impl(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state, rq_policy* policy,
                        rq_rng* rng, uint32_t n_steps, int mode, uint32_t flags, rq_trajectory* traj,
                        const rq_reference* ref = nullptr, const rq_reference_bank* refs = nullptr,
                        const uint32_t* reference_id = nullptr) {
    RolloutFrame f;
    const bool tracked = ref || refs;
    int rc = rollout_check(f, dev, env, params, state, rng, policy != nullptr, n_steps, mode, flags, traj); if (rc) return rc;
    RQ_REQUIRE(policy->dev == dev, RQ_ERR_SHAPE_MISMATCH, "policy lives on another device");
    if (tracked) {      // a tracked rollout is refused here, before anything is enqueued
        if (ref) { rc = rollout_check_reference(__func__, dev, env, ref); if (rc) return rc; }
        rc = rollout_check_reference_bank(__func__, dev, env, refs, reference_id); if (rc) return rc;
        RQ_REQUIRE(policy->sas_mode == RQ_SAS_OFF, RQ_ERR_INVALID_ARGUMENT,
                   "tracked rollouts do not carry the SampleAndSquash stage");
    }
    if (f.wr.rows && mode == RQ_ROLLOUT_FUSED) {        // a schedule is flown fused by the fp32 builds alone; nothing runs chained in its place
        if (policy->precision != RQ_POLICY_FP32) return wrench_refuses_fused(__func__, "a bf16 / f16x2 policy");
        if (policy->sas_mode != RQ_SAS_OFF) return wrench_refuses_fused(__func__, "a policy with a SampleAndSquash stage");
    }
    const uint32_t interval = policy->native_interval;      // above 1: the RATE kernels (a SampleAndSquash stage cannot be set beside it)
    DeviceScope on_device(dev); rc = on_device.rc; if (rc) return rc;
    rc = policy_size(policy, env->n); if (rc) return rc;
    RQ_REQUIRE(policy->ld == env->ld, RQ_ERR_SHAPE_MISMATCH, "policy batch does not match the env");
    rc = rollout_track(f, env, ref); if (rc) return rc;
    rc = rollout_track_refs(f, dev, env, refs, reference_id); if (rc) return rc;
    rc = rollout_begin(f, dev, env, state, n_steps, flags, traj); if (rc) return rc;
    if (mode == RQ_ROLLOUT_FUSED) {
        unsigned long long* span = nullptr;
        rc = fused_span_begin(__func__, dev, env, n_steps, &span); if (rc) return rc;
        rq::FusedArgs a = fused_args(f, env, params, state, rng, n_steps, flags, span);
        a.hidden = policy->hidden; a.weights = policy->w_dev;
        a.precision = policy->precision; a.images = packed_of(policy); a.interval = interval;
        a.sas = sas_of(policy, rng->epoch, nullptr, env->offset);
        RQ_HIP(rq::launch_rollout_fused(dev->stream, a));
        fused_span_end(dev, n_steps);
    } else {
        // one step = observe -> evaluate_step -> step (-> record) on the stream.  Without a recording the step kernel
        // also assembles the NEXT step's observation (round 3: two launches per step instead of three; the first
        // observation of the rollout is a launch of its own, the one assembled by the last step is not used)
        // A tracked rollout puts one small kernel in front of the actor: it takes the setpoint off the assembled observation,
        // wherever that came from, and keeps the tracking error (the observation the last step assembles is never shifted).
        const uint32_t step_nodes = tracked ? 3u : 2u;
        const bool fold_observe = traj == nullptr;
        auto enqueue_step = [&](uint32_t epoch, const uint32_t* epoch_base, uint32_t t_record) -> hipError_t {
            hipError_t e = hipSuccess;
            if (!fold_observe)
                e = rq::launch_observe(dev->stream, f.b, f.nc, f.noise, rng->seed, epoch, epoch_base, params->d, state->d, env->obs);
            if (e == hipSuccess && tracked)
                e = rq::launch_track_shift(dev->stream, f.b, state->d, env->st, env->obs, f.trk);
            if (e == hipSuccess && interval > 1)     // the env's episode step count is that of this step's observation: k_step moves it on
                e = rq::launch_actor_step_rate(dev->stream, env->n, packed_of(policy), env->obs, env->ld, policy->hidden,
                                               policy->ld, env->act, env->ld, env->st.frozen, policy->precision, env->st.steps,
                                               interval, 0u);
            else if (e == hipSuccess)
                e = rq::launch_actor_step(dev->stream, env->n, packed_of(policy), env->obs, env->ld, policy->hidden,
                                          policy->ld, env->act, env->ld, env->st.frozen, policy->precision,
                                          sas_of(policy, epoch, epoch_base, env->offset));
            if (e == hipSuccess)
                e = rq::launch_step(dev->stream, f.b, f.sc, params->d, state->d, env->act, state->d, env->st,
                                    /*rollout=*/1, flags, f.smp, rng->seed, policy->hidden, policy->w_dev, rq::Mailbox{},
                                    fold_observe ? env->obs : nullptr, f.nc, f.noise, epoch + 1, epoch_base, f.wr);
            if (e == hipSuccess && traj) {
                rq::TrajPtrs tt = f.tp; tt.t0 = f.tp.t0 + t_record;
                e = rq::launch_record(dev->stream, f.b, env->obs, env->act, env->st, tt);
            }
            return e;
        };
        if (n_steps && (flags & RQ_ROLLOUT_AUTORESET))   // envs frozen by an earlier rollout start their next episode
            RQ_HIP(rq::launch_thaw_frozen(dev->stream, f.b, f.smp, rng->seed, params->d, state->d, env->st, policy->hidden,
                                          policy->w_dev));
        if (fold_observe && n_steps)     // the rollout's first observation (after the thaw: of the re-sampled states)
            RQ_HIP(rq::launch_observe(dev->stream, f.b, f.nc, f.noise, rng->seed, rng->epoch, nullptr, params->d, state->d, env->obs));
        uint32_t done_steps = 0;
        if (!traj && n_steps >= kGraphSteps) {
            // replay a captured graph of kGraphSteps steps; kernel boundaries stay (~1.5 us each) but the
            // host no longer pays ~3.5 us per launch, which is what bounds small batches
            rq_env::GraphKey key;      // what the graph's nodes carry by value: another value of any of these is another graph
            key.params = params->d; key.state = state->d; key.hidden = policy->hidden; key.packed = packed_of(policy);
            key.weights = policy->w_dev; key.obs = env->obs; key.flags = flags; key.precision = policy->precision; key.cfg = env->cfg;
            key.seed = rng->seed; key.sas_mode = policy->sas_mode; key.sas_seed = policy->sas_seed; key.ls_image = policy->ls_image;
            key.ref = f.trk.ref; key.ref_rows = f.trk.rows; key.row0_at = f.trk.row0_at;
            key.row0_gen = f.row0_gen;      // (a reference bank: which ids the rows were built from)
            key.interval = interval; key.wrench_gen = env->wrench_gen;
            hipGraphExec_t exec = nullptr;
            for (auto& g : env->graphs)
                if (g.key == key) { exec = g.exec; break; }
            if (!exec) {
                // Built node by node (rq_kernels.hpp GraphSink), NOT by stream capture: while any stream of a process captures, HIP
                // fails hipDeviceSynchronize on every other thread (hipErrorStreamCaptureUnsupported) and invalidates the capture -
                // a learner's PyTorch thread on the same GPU broke the rollout and was broken by it (tools/foreign_soak.py, round 6).
                // Should the construction fail all the same, the steps go out as plain launches: same kernels, same order.
                hipGraph_t graph = nullptr;
                hipError_t ce = dev->graphs_enabled ? hipGraphCreate(&graph, 0) : hipErrorNotSupported;
                if (ce == hipSuccess) {
                    rq::GraphSink sink;
                    sink.graph = graph;
                    rq::set_graph_sink(&sink);
                    for (uint32_t t = 0; t < kGraphSteps && ce == hipSuccess; ++t) ce = enqueue_step(t, env->epoch_dev, 0);
                    if (ce == hipSuccess) ce = rq::launch_add_u32(dev->stream, env->epoch_dev, kGraphSteps);
                    rq::set_graph_sink(nullptr);
                    if (ce == hipSuccess && sink.nodes != step_nodes * kGraphSteps + 1) ce = hipErrorUnknown;     // a launcher that bypassed the sink
                }
                if (ce == hipSuccess) ce = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
                if (graph) (void)hipGraphDestroy(graph);
                if (ce != hipSuccess) {
                    (void)hipGetLastError();         // the failed construction's; the direct launches below report their own
                    exec = nullptr;
                    ++dev->graph_fallbacks;
                } else {
                    if (env->graphs.size() >= kMaxGraphs) {        // least recently created goes (a replay is cheap to rebuild)
                        RQ_HIP(hipStreamSynchronize(dev->stream));
                        (void)hipGraphExecDestroy(env->graphs.front().exec);
                        env->graphs.erase(env->graphs.begin());
                    }
                    try {                       // nothing throws across the boundary
                        env->graphs.push_back({key, exec});
                    } catch (const std::bad_alloc&) {
                        (void)hipGraphExecDestroy(exec);
                        return fail(RQ_ERR_OUT_OF_MEMORY, "rollout: host allocation failed");
                    }
                }
            }
            if (exec) {
                RQ_HIP(rq::launch_set_u32(dev->stream, env->epoch_dev, rng->epoch));
                for (; done_steps + kGraphSteps <= n_steps; done_steps += kGraphSteps)
                    RQ_HIP(hipGraphLaunch(exec, dev->stream));
            }
        }
        for (uint32_t t = done_steps; t < n_steps; ++t) RQ_HIP(enqueue_step(rng->epoch + t, nullptr, t));
    }
    rollout_end(state, rng, n_steps, traj);
    return RQ_OK;
}

RQ_API int rq_rollout(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state, rq_policy* policy,
               rq_rng* rng, uint32_t n_steps, int mode, uint32_t flags) {
    return rollout_impl(dev, env, params, state, policy, rng, n_steps, mode, flags, nullptr);
}

RQ_API int rq_rollout_record(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state, rq_policy* policy,
                      rq_rng* rng, uint32_t n_steps, int mode, uint32_t flags, rq_trajectory* trajectory) {
    RQ_REQUIRE(trajectory, RQ_ERR_INVALID_ARGUMENT, "null trajectory");
    return rollout_impl(dev, env, params, state, policy, rng, n_steps, mode, flags, trajectory);
}

// ---------------------------------------------------------------------------- Tracking
RQ_API int rq_reference_create(rq_device* dev, const float* host_rows, uint32_t rows, rq_reference** out) {
    RQ_REQUIRE(dev && host_rows && out, RQ_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    RQ_REQUIRE(rows > 0, RQ_ERR_INVALID_ARGUMENT, "a reference needs at least one row");
    for (size_t j = 0; j < (size_t)rows * 6; ++j)
        RQ_REQUIRE(std::isfinite(host_rows[j]), RQ_ERR_INVALID_ARGUMENT, "reference holds a non-finite entry");
    DeviceScope on_device(dev); int rc = on_device.rc; if (rc) return rc;
    rq_reference* r = new (std::nothrow) rq_reference();
    RQ_REQUIRE(r, RQ_ERR_OUT_OF_MEMORY, "host allocation failed");
    r->dev = dev; r->ordinal = dev->ordinal; r->rows = rows;
    if (r->d.alloc((size_t)rows * 6) != hipSuccess) {
        delete r;
        return fail(RQ_ERR_OUT_OF_MEMORY, "rq_reference_create: device allocation failed");
    }
    // (synchronous: the caller's rows are its own again on return)
    const hipError_t e = hipMemcpy(r->d, host_rows, (size_t)rows * 6 * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        delete r;
        return fail(RQ_ERR_HIP, std::string("rq_reference_create: hipMemcpy -> ") + hipGetErrorString(e));
    }
    *out = r;
    return RQ_OK;
}

RQ_API int rq_reference_destroy(rq_reference* reference) {
    if (!reference) return RQ_OK;
    DeviceScope on_device(reference->ordinal);     // (hipFree synchronises the device: no launch still reads the table)
    delete reference;
    return RQ_OK;
}

RQ_API int rq_rollout_track(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state, rq_policy* policy,
                     rq_rng* rng, uint32_t n_steps, int mode, uint32_t flags, rq_trajectory* trajectory,
                     const rq_reference* reference) {
    RQ_REQUIRE(reference, RQ_ERR_INVALID_ARGUMENT, "null reference");
    return rollout_impl(dev, env, params, state, policy, rng, n_steps, mode, flags, trajectory, reference);
}

RQ_API int rq_reference_bank_create(rq_device* dev, const float* host_rows, uint32_t n_refs, uint32_t rows, rq_reference_bank** out) {
    RQ_REQUIRE(dev && host_rows && out, RQ_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    RQ_REQUIRE(n_refs > 0 && rows > 0, RQ_ERR_INVALID_ARGUMENT, "a reference bank needs at least one table of at least one row");
    // the row an env reads, first row of its table + episode step count, is a uint32 on the device
    RQ_REQUIRE((uint64_t)n_refs * rows < (1ull << 28), RQ_ERR_INVALID_ARGUMENT, "a reference bank holds fewer than 2^28 rows in all");
    const size_t floats = (size_t)n_refs * rows * 6;
    for (size_t j = 0; j < floats; ++j)
        RQ_REQUIRE(std::isfinite(host_rows[j]), RQ_ERR_INVALID_ARGUMENT,
                   "reference bank holds a non-finite entry: table " + std::to_string(j / ((size_t)rows * 6)) + ", row " +
                       std::to_string(j / 6 % rows));
    DeviceScope on_device(dev); int rc = on_device.rc; if (rc) return rc;
    rq_reference_bank* r = new (std::nothrow) rq_reference_bank();
    RQ_REQUIRE(r, RQ_ERR_OUT_OF_MEMORY, "host allocation failed");
    r->dev = dev; r->ordinal = dev->ordinal; r->n_refs = n_refs; r->rows = rows;
    if (r->d.alloc(floats) != hipSuccess) {
        delete r;
        return fail(RQ_ERR_OUT_OF_MEMORY, "rq_reference_bank_create: device allocation failed");
    }
    // (synchronous: the caller's rows are its own again on return)
    const hipError_t e = hipMemcpy(r->d, host_rows, floats * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        delete r;
        return fail(RQ_ERR_HIP, std::string("rq_reference_bank_create: hipMemcpy -> ") + hipGetErrorString(e));
    }
    *out = r;
    return RQ_OK;
}

RQ_API int rq_reference_bank_destroy(rq_reference_bank* references) {
    if (!references) return RQ_OK;
    DeviceScope on_device(references->ordinal);     // (hipFree synchronises the device: no launch still reads the tables)
    delete references;
    return RQ_OK;
}

// ---------------------------------------------------------------------------- Wrench schedule
RQ_API int rq_wrench_bank_create(rq_device* dev, const float* host_rows, uint32_t n_tables, uint32_t rows, int units, rq_wrench_bank** out) {
    RQ_REQUIRE(dev && host_rows && out, RQ_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    RQ_REQUIRE(n_tables > 0 && rows > 0, RQ_ERR_INVALID_ARGUMENT, "a wrench bank needs at least one table of at least one row");
    // the row an env reads, first row of its table + episode step count, is a uint32 on the device
    RQ_REQUIRE((uint64_t)n_tables * rows < (1ull << 28), RQ_ERR_INVALID_ARGUMENT, "a wrench bank holds fewer than 2^28 rows in all");
    RQ_REQUIRE(units == RQ_WRENCH_RELATIVE || units == RQ_WRENCH_ABSOLUTE, RQ_ERR_INVALID_ARGUMENT,
               "unknown units: RQ_WRENCH_RELATIVE or RQ_WRENCH_ABSOLUTE");
    const size_t floats = (size_t)n_tables * rows * 6;
    for (size_t j = 0; j < floats; ++j)
        RQ_REQUIRE(std::isfinite(host_rows[j]), RQ_ERR_INVALID_ARGUMENT,
                   "wrench bank holds a non-finite entry: table " + std::to_string(j / ((size_t)rows * 6)) + ", row " +
                       std::to_string(j / 6 % rows));
    DeviceScope on_device(dev); int rc = on_device.rc; if (rc) return rc;
    rq_wrench_bank* r = new (std::nothrow) rq_wrench_bank();
    RQ_REQUIRE(r, RQ_ERR_OUT_OF_MEMORY, "host allocation failed");
    r->dev = dev; r->ordinal = dev->ordinal; r->n_tables = n_tables; r->rows = rows; r->units = units;
    if (r->d.alloc(floats) != hipSuccess) {
        delete r;
        return fail(RQ_ERR_OUT_OF_MEMORY, "rq_wrench_bank_create: device allocation failed");
    }
    // (synchronous: the caller's rows are its own again on return)
    const hipError_t e = hipMemcpy(r->d, host_rows, floats * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        delete r;
        return fail(RQ_ERR_HIP, std::string("rq_wrench_bank_create: hipMemcpy -> ") + hipGetErrorString(e));
    }
    *out = r;
    return RQ_OK;
}

RQ_API int rq_wrench_bank_destroy(rq_wrench_bank* bank) {
    if (!bank) return RQ_OK;
    RQ_REQUIRE(bank->attached == 0, RQ_ERR_INVALID_ARGUMENT,
               "the wrench bank is attached to " + std::to_string(bank->attached) +
                   " live env(s): detach it (rq_env_set_wrench_schedule with a NULL bank) or destroy the env first");
    DeviceScope on_device(bank->ordinal);     // (hipFree synchronises the device: no launch still reads the tables)
    delete bank;
    return RQ_OK;
}

RQ_API int rq_env_set_wrench_schedule(rq_env* env, rq_wrench_bank* bank, const uint32_t* wrench_id) {
    RQ_REQUIRE(env, RQ_ERR_INVALID_ARGUMENT, "null argument");
    rq_device* dev = env->dev;
    if (bank) {
        RQ_REQUIRE(bank->dev == dev, RQ_ERR_SHAPE_MISMATCH, "wrench bank lives on another device");
        if (wrench_id)
            for (uint32_t i = 0; i < env->n; ++i)
                RQ_REQUIRE(wrench_id[i] < bank->n_tables, RQ_ERR_INVALID_ARGUMENT,
                           "wrench id out of range: env " + std::to_string(i) + " names table " + std::to_string(wrench_id[i]) +
                               " of a bank of " + std::to_string(bank->n_tables));
    }
    DeviceScope on_device(dev); int rc = on_device.rc; if (rc) return rc;      // (retires a running resident executor)
    RQ_HIP(hipStreamSynchronize(dev->stream));                // a launch in flight reads the rows of the schedule before
    obs_cache_drop_if(dev, env);
    if (!bank) {
        if (env->wrench) env->wrench->attached -= 1;
        env->wrench = nullptr; env->wrench_gen = 0; env->wrench_ids.clear();
        return RQ_OK;
    }
    std::vector<uint32_t> ids, first;
    try {                                   // nothing throws across the boundary
        if (wrench_id) ids.assign(wrench_id, wrench_id + env->n); else ids.assign(env->n, 0u);
        first.assign(env->ld, 0u);
    } catch (const std::bad_alloc&) {
        return fail(RQ_ERR_OUT_OF_MEMORY, "wrench schedule: host allocation failed");
    }
    for (uint32_t i = 0; i < env->n; ++i) first[i] = ids[i] * bank->rows;       // < n_tables * rows < 2^28
    if (env->wrench_row0.empty() && env->wrench_row0.alloc(env->ld) != hipSuccess)
        return fail(RQ_ERR_OUT_OF_MEMORY, "wrench schedule: device allocation failed");
    // (synchronous: `first` is pageable and goes away)
    RQ_HIP(hipMemcpy(env->wrench_row0, first.data(), (size_t)env->ld * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (env->wrench) env->wrench->attached -= 1;
    bank->attached += 1;
    env->wrench = bank;
    env->wrench_ids.swap(ids);
    env->wrench_gen = fresh_version();
    return RQ_OK;
}

RQ_API int rq_env_get_wrench_schedule(const rq_env* env, rq_wrench_bank** bank, uint32_t* wrench_id_out) {
    RQ_REQUIRE(env && bank, RQ_ERR_INVALID_ARGUMENT, "null argument");
    *bank = env->wrench;
    if (env->wrench && wrench_id_out) std::memcpy(wrench_id_out, env->wrench_ids.data(), (size_t)env->n * sizeof(uint32_t));
    return RQ_OK;
}

RQ_API int rq_rollout_track_refs(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state, rq_policy* policy,
                                 rq_rng* rng, uint32_t n_steps, int mode, uint32_t flags, rq_trajectory* trajectory,
                                 const rq_reference_bank* references, const uint32_t* reference_id) {
    RQ_REQUIRE(references, RQ_ERR_INVALID_ARGUMENT, "null reference bank");
    RQ_REQUIRE(reference_id, RQ_ERR_INVALID_ARGUMENT, "null reference_id");
    return rollout_impl(dev, env, params, state, policy, rng, n_steps, mode, flags, trajectory, nullptr, references, reference_id);
}

// ---------------------------------------------------------------------------- Trajectory
RQ_API int rq_trajectory_create(rq_env* env, uint32_t capacity_steps, rq_trajectory** out) {
    RQ_REQUIRE(env && out, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(capacity_steps > 0, RQ_ERR_INVALID_ARGUMENT, "capacity must be positive");
    // one step of the observation block is addressed with 32-bit buffer offsets (k_rollout_fused)
    RQ_REQUIRE((uint64_t)env->ld * RQ_POLICY_INPUT_DIM * sizeof(float) < (1ull << 32), RQ_ERR_INVALID_ARGUMENT,
               "trajectory recording supports up to 48 million envs per device");
    *out = nullptr;
    DeviceScope on_device(env->dev); int rc = on_device.rc; if (rc) return rc;
    rq_trajectory* t = new (std::nothrow) rq_trajectory();
    RQ_REQUIRE(t, RQ_ERR_OUT_OF_MEMORY, "host allocation failed");
    t->env = env; t->ordinal = env->ordinal; t->capacity = capacity_steps;
    const size_t per = (size_t)capacity_steps * env->ld;
    if (t->obs.alloc(per * RQ_POLICY_INPUT_DIM) != hipSuccess || t->act.alloc(per * RQ_ACTION_DIM) != hipSuccess ||
        t->rew.alloc(per) != hipSuccess || t->done.alloc(per) != hipSuccess) {
        delete t;
        return fail(RQ_ERR_OUT_OF_MEMORY, "rq_trajectory_create: device allocation failed");
    }
    *out = t;
    return RQ_OK;
}

RQ_API int rq_trajectory_destroy(rq_trajectory* t) {
    if (!t) return RQ_OK;
    DeviceScope on_device(t->ordinal);
    delete t;
    return RQ_OK;
}

RQ_API int rq_trajectory_reset(rq_trajectory* t) {
    RQ_REQUIRE(t, RQ_ERR_INVALID_ARGUMENT, "null argument");
    t->length = 0;
    t->grad.valid = false;
    return RQ_OK;
}

RQ_API int rq_trajectory_length(const rq_trajectory* t, uint32_t* steps, uint32_t* capacity) {
    RQ_REQUIRE(t, RQ_ERR_INVALID_ARGUMENT, "null argument");
    if (steps) *steps = t->length;
    if (capacity) *capacity = t->capacity;
    return RQ_OK;
}

RQ_API int rq_trajectory_device_ptrs(const rq_trajectory* t, float** obs, float** act, float** rew, uint8_t** done,
                              uint32_t* ld) {
    RQ_REQUIRE(t, RQ_ERR_INVALID_ARGUMENT, "null argument");
    if (obs) *obs = t->obs;
    if (act) *act = t->act;
    if (rew) *rew = t->rew;
    if (done) *done = t->done;
    if (ld) *ld = t->env->ld;
    return RQ_OK;
}

// host copies, learner layout: obs [T, N, 22], act [T, N, 4], rew [T, N], done [T, N]; any pointer may be NULL
// [steps][dim][ld] on the device -> host [steps][n][dim]: one layout launch per chunk of steps, one copy
RQ_API int rq_trajectory_get(const rq_trajectory* t, float* obs, float* act, float* rew, uint8_t* done) {
    RQ_REQUIRE(t, RQ_ERR_INVALID_ARGUMENT, "null argument");
    rq_env* env = t->env;
    rq_device* dev = env->dev;
    const uint32_t n = env->n, ld = env->ld;
    DeviceScope on_device(dev); int rc = on_device.rc; if (rc) return rc;
    if (t->length == 0) return RQ_OK;
    if (obs) { rc = traj_block_to_host(dev, t->obs, t->length, n, ld, RQ_POLICY_INPUT_DIM, obs); if (rc) return rc; }
    if (act) { rc = traj_block_to_host(dev, t->act, t->length, n, ld, RQ_ACTION_DIM, act); if (rc) return rc; }
    if (rew) { rc = traj_block_to_host(dev, t->rew, t->length, n, ld, 1, rew); if (rc) return rc; }
    if (done) {
        RQ_HIP(hipMemcpy2DAsync(done, n, t->done, ld, n, t->length, hipMemcpyDeviceToHost, dev->stream));
        RQ_HIP(hipStreamSynchronize(dev->stream));
    }
    return RQ_OK;
}

RQ_API int rq_trajectory_relabel(rq_trajectory* t, rq_policy* pol, float* action_out, int overwrite) {
    RQ_REQUIRE(t && pol, RQ_ERR_INVALID_ARGUMENT, "null argument");
    rq_env* env = t->env;
    rq_device* dev = env->dev;
    RQ_REQUIRE(pol->dev == dev, RQ_ERR_SHAPE_MISMATCH, "policy lives on another device");
    RQ_REQUIRE(pol->sas_mode != RQ_SAS_SAMPLE, RQ_ERR_INVALID_ARGUMENT,
               "relabelling is a deterministic pass: RQ_SAS_SAMPLE is defined for evaluate_step and rollouts");
    { const int rate_rc = require_native_rate(pol, "rq_trajectory_relabel"); if (rate_rc) return rate_rc; }
    if (t->length == 0) return RQ_OK;
    DeviceScope on_device(dev); int rc = on_device.rc; if (rc) return rc;
    rc = policy_size(pol, env->n); if (rc) return rc;
    float* d_act = t->act;
    if (!overwrite) {
        RQ_HIP(dev->rows2.reserve(dev->stream, (size_t)t->length * RQ_ACTION_DIM * env->ld));
        d_act = dev->rows2;
    }
    RQ_HIP(rq::launch_actor_relabel(dev->stream, env->n, env->ld, t->length, packed_of(pol), t->obs, t->done, pol->hidden,
                                    pol->ld, d_act, mode_of(pol)));
    if (action_out) return traj_block_to_host(dev, d_act, t->length, env->n, env->ld, RQ_ACTION_DIM, action_out);
    return RQ_OK;
}

}  // extern "C"
