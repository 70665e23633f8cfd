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
int rollout_check(RolloutFrame& f, const RolloutCall& c, bool actor) {
    const rq_trajectory* traj = c.traj;
    int rc = check_env_objects(c.dev, c.env, c.params, c.state); if (rc) return rc;
    RQ_REFUSE(c.who, c.params && c.state && actor && c.rng, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REFUSE(c.who, c.rng->initialized, RQ_ERR_NOT_INITIALIZED, "initialize_rng was not called");
    RQ_REFUSE(c.who, c.mode == RQ_ROLLOUT_FUSED || c.mode == RQ_ROLLOUT_CHAINED, RQ_ERR_INVALID_ARGUMENT, "unknown mode");
    RQ_REFUSE(c.who, (c.flags & ~(uint32_t)RQ_ROLLOUT_AUTORESET) == 0, RQ_ERR_INVALID_ARGUMENT, "unknown flags");
    if (traj) {
        RQ_REFUSE(c.who, traj->env == c.env, RQ_ERR_SHAPE_MISMATCH, "trajectory belongs to another env");
        RQ_REFUSE(c.who, (uint64_t)traj->length + c.n_steps <= traj->capacity, RQ_ERR_INVALID_ARGUMENT,
                  "trajectory buffer too small for this rollout");
        f.tp = {traj->obs, traj->act, traj->rew, traj->done, traj->length};
    }
    // A schedule is flown fused by the fp32 builds alone and without another schedule beside it; nothing runs chained in its place
    // (the actors refuse what is theirs: a 16-bit policy, a SampleAndSquash stage, a teacher bank).  Kind by kind, each refused beside
    // the kinds before it, earliest first.
    rc = env_schedules("rollout", c.env, f.sched); if (rc) return rc;
    for (int k = 0; k < kScheduleKinds && c.mode == RQ_ROLLOUT_FUSED; ++k)
        for (int j = 0; j < k && f.sched[k].rows; ++j)
            if (f.sched[j].rows)
                return refuses_fused(c.who, k, (std::string("an env that carries a ") + kTableKinds[j].noun + " schedule too").c_str());
    return RQ_OK;
}

int schedule_too_short(const char* who, const rq_env* env, int kind) {
    return fail(RQ_ERR_INVALID_ARGUMENT, std::string(who) + ": the env's " + kTableKinds[kind].noun + " schedule has fewer rows (" +
                                             std::to_string(env->schedule[kind].bank->rows) + ") than episode_step_limit (" +
                                             std::to_string(env->cfg.episode_step_limit) + "): every table must cover an episode");
}

int refuses_fused(const char* who, int kind, const char* what) {
    return fail(RQ_ERR_INVALID_ARGUMENT, std::string(who) + ": the env carries a " + kTableKinds[kind].noun +
                                             " schedule, which the fused kernel of " + what +
                                             " is not taught: fly it with mode RQ_ROLLOUT_CHAINED (\"chained\"), or detach the schedule");
}

int rollout_check_tables(const RolloutCall& c) {
    const RowTables* t = c.tables;
    if (!t) return RQ_OK;
    const char* noun = c.reference_id ? "reference bank" : "reference";
    RQ_REFUSE(c.who, t->dev == c.dev, RQ_ERR_SHAPE_MISMATCH, std::string(noun) + " lives on another device");
    RQ_REFUSE(c.who, t->rows >= c.env->cfg.episode_step_limit, RQ_ERR_INVALID_ARGUMENT,
              std::string(noun) + " has fewer rows than episode_step_limit: " + (c.reference_id ? "every" : "the") + " table must cover an episode");
    for (uint32_t i = 0; c.reference_id && i < c.env->n; ++i)
        RQ_REFUSE(c.who, c.reference_id[i] < t->n_tables, RQ_ERR_INVALID_ARGUMENT,
                  "reference id out of range: env " + std::to_string(i) + " names reference " + std::to_string(c.reference_id[i]) +
                      " of a bank of " + std::to_string(t->n_tables));
    return RQ_OK;
}

int first_rows_failed(const char* what, const rq::FirstRowsStatus& s) {
    switch (s.what) {
    case rq::FirstRowsStatus::host_allocation: return fail(RQ_ERR_OUT_OF_MEMORY, std::string(what) + ": host allocation failed");
    case rq::FirstRowsStatus::device_allocation: return fail(RQ_ERR_OUT_OF_MEMORY, std::string(what) + ": device allocation failed");
    case rq::FirstRowsStatus::copy: return hip_failed("upload_first_rows", "hipMemcpyAsync", s.hip);
    case rq::FirstRowsStatus::synchronize: return hip_failed("upload_first_rows", "hipStreamSynchronize", s.hip);
    case rq::FirstRowsStatus::zero: return hip_failed("DelayHistory::attach", "hipMemsetAsync", s.hip);
    default: return RQ_OK;
    }
}

int rollout_track(RolloutFrame& f, const RolloutCall& c) {
    const RowTables* t = c.tables;
    if (!t) return RQ_OK;
    rq_env* env = c.env;
    int rc = env_track_stats(env, &f.trk.sq, &f.trk.steps); if (rc) return rc;
    f.trk.ref = t->d; f.trk.rows = t->rows;
    if (!c.reference_id) return RQ_OK;      // one reference: no first rows (row0_at 0, row0_gen 0)
    // The env caches what its first rows (the block's third array) were built from, as the policy bank caches its id table: a loop of
    // rollouts with one assignment uploads them once; other ids wait for the stream, then rewrite the rows.
    const uint32_t n = env->n;
    const bool same = env->row0_valid && env->row0_key == t->uid && env->row0_ids.size() == n &&
                      std::memcmp(env->row0_ids.data(), c.reference_id, (size_t)n * sizeof(uint32_t)) == 0;
    if (!same) {
        env->row0_valid = false;
        try {                                   // nothing throws across the boundary
            env->row0_ids.assign(c.reference_id, c.reference_id + n);
        } catch (const std::bad_alloc&) {
            return fail(RQ_ERR_OUT_OF_MEMORY, "reference bank: host allocation failed");
        }
        RQ_HIP(hipStreamSynchronize(c.dev->stream));              // a rollout in flight reads the rows of the ids before
        const rq::FirstRowsStatus up = rq::upload_first_rows(c.dev->stream, c.reference_id, n, env->ld, t->rows, f.trk.steps + env->ld);
        if (up) return first_rows_failed("reference bank", up);
        env->row0_valid = true;
        env->row0_key = t->uid;
        env->row0_gen = fresh_version();
    }
    f.trk.row0_at = env->ld; f.row0_gen = env->row0_gen;
    return RQ_OK;
}

int rollout_begin(RolloutFrame& f, const RolloutCall& c) {
    rq_env* env = c.env;
    obs_cache_drop_if(c.dev, env);
    if (c.n_steps) { const int rc = state_make_private(c.state, true); if (rc) return rc; }      // steps the state in place
    f.b = batch_of(env);
    f.sc = rq::step_cfg(env->cfg);
    f.nc = rq::noise_cfg(env->cfg);
    f.smp = rq::sample_cfg(env->cfg);
    f.noise = rq::noise_enabled(env->cfg);
    if (c.traj && c.n_steps && !(c.flags & RQ_ROLLOUT_AUTORESET))   // steps a frozen wave never reaches read as "not stepped"
        RQ_HIP(hipMemsetAsync(c.traj->done + (size_t)c.traj->length * env->ld, 4, (size_t)c.n_steps * env->ld, c.dev->stream));
    return RQ_OK;
}

void rollout_end(const RolloutCall& c) {
    c.rng->epoch += c.n_steps;
    if (c.traj) c.traj->length += c.n_steps;
    if (c.n_steps) c.state->version = fresh_version();
}

rq::FusedArgs fused_args(const RolloutCall& c, const RolloutFrame& f) {
    rq::FusedArgs a;
    a.b = f.b; a.c = f.sc; a.nc = f.nc; a.sc = f.smp; a.noise = f.noise;
    a.seed = c.rng->seed; a.epoch0 = c.rng->epoch; a.n_steps = c.n_steps;
    a.autoreset = (c.flags & RQ_ROLLOUT_AUTORESET) != 0;
    a.params = c.params->d; a.state = c.state->d; a.st = c.env->st;
    a.traj = f.tp; a.trk = f.trk; set_schedules(a, f.sched);
    return a;
}

rq::EnvStepLaunch env_step_launch(const RolloutCall& c, const RolloutFrame& f) {
    rq::EnvStepLaunch e;
    e.b = f.b; e.c = f.sc; e.params = c.params->d; e.state = c.state->d; e.action = c.env->act; e.next_state = c.state->d; e.st = c.env->st;
    e.rollout = true; e.flags = c.flags; e.sc = f.smp; e.seed = c.rng->seed; set_schedules(e, f.sched);
    return e;
}

int fused_launch(const RolloutCall& c, rq::FusedArgs& a) {
    rq_device* dev = c.dev;
    if (dev->k_timing && c.n_steps) {                   // one (in, out) record per wave = per workgroup of the fused kernel
        const uint32_t waves = (c.env->n + 63u) / 64u;
        const hipError_t e = dev->k_span.reserve(dev->stream, (size_t)waves * 5);
        if (e != hipSuccess) return hip_failed(c.who, "dev->k_span.reserve(dev->stream, (size_t)waves * 5)", e);
        dev->k_span_used = waves;
    }
    a.span = dev->k_timing ? dev->k_span.get() : nullptr;
    const hipError_t e = rq::launch_rollout_fused(dev->stream, a);
    if (e != hipSuccess) return hip_failed(c.who, "rq::launch_rollout_fused", e);
    dev->k_timed = dev->k_timing && c.n_steps > 0;
    dev->k_fetched = false;
    return RQ_OK;
}

}  // namespace rqh

using namespace rqh;

// ---------------------------------------------------------------------------- Rollout ---
namespace {

// One policy flies every env.  Its chained launches fold the observe into the step and replay as a hipGraph (rollout_chained); a
// native interval above 1 takes the RATE kernels (a SampleAndSquash stage cannot be set beside it).
struct PolicyActor {
    static constexpr bool kFoldAndReplay = true;
    rq_policy* policy;
    bool given() const { return policy != nullptr; }
    int check(const RolloutCall& c, const RolloutFrame& f) const {
        RQ_REFUSE(c.who, policy->dev == c.dev, RQ_ERR_SHAPE_MISMATCH, "policy lives on another device");
        RQ_REFUSE(c.who, !c.tables || policy->sas_mode == RQ_SAS_OFF, RQ_ERR_INVALID_ARGUMENT,
                  "tracked rollouts do not carry the SampleAndSquash stage");
        for (int k = 0; k < kScheduleKinds && c.mode == RQ_ROLLOUT_FUSED; ++k) {      // a schedule is flown fused by the fp32 builds alone
            if (!f.sched[k].rows) continue;
            if (policy->precision != RQ_POLICY_FP32) return refuses_fused(c.who, k, "a bf16 / f16x2 policy");
            if (policy->sas_mode != RQ_SAS_OFF) return refuses_fused(c.who, k, "a policy with a SampleAndSquash stage");
        }
        return RQ_OK;
    }
    int prepare(const RolloutCall& c) const {
        const int rc = policy_size(policy, c.env->n); if (rc) return rc;
        RQ_REFUSE(c.who, policy->ld == c.env->ld, RQ_ERR_SHAPE_MISMATCH, "policy batch does not match the env");
        return RQ_OK;
    }
    int fused(const RolloutCall& c, const RolloutFrame& f) const {
        rq::FusedArgs a = fused_args(c, f);
        a.hidden = policy->hidden; a.weights = policy->w_dev;
        a.precision = policy->precision; a.images = packed_of(policy); a.interval = policy->native_interval;
        a.sas = sas_of(policy, c.rng->epoch, nullptr, c.env->offset);
        return fused_launch(c, a);
    }
    rq::EnvStepLaunch env_step(const RolloutCall& c, const RolloutFrame& f) const {
        rq::EnvStepLaunch e = env_step_launch(c, f);
        e.hidden = policy->hidden; e.weights = policy->w_dev;
        return e;
    }
    hipError_t thaw(const RolloutCall& c, const RolloutFrame& f) const { return rq::launch_thaw_frozen(c.dev->stream, env_step(c, f)); }
    hipError_t act(const RolloutCall& c, const RolloutFrame&, uint32_t epoch, const uint32_t* epoch_base) const {
        const rq_env* env = c.env;
        rq::ActorStepLaunch a;
        a.n = env->n; a.packed = packed_of(policy); a.precision = policy->precision;
        a.obs = env->obs; a.ld_obs = env->ld; a.hidden = policy->hidden; a.ld_h = policy->ld; a.act = env->act; a.ld_act = env->ld;
        a.frozen = env->st.frozen;
        a.sas = sas_of(policy, epoch, epoch_base, env->offset);      // (off under a native interval above 1)
        a.steps = env->st.steps; a.interval = policy->native_interval;
        return rq::launch_actor_step(c.dev->stream, a);
    }
    hipError_t step(const RolloutCall& c, const RolloutFrame& f, uint32_t epoch, const uint32_t* epoch_base, bool fold) const {
        rq::EnvStepLaunch e = env_step(c, f);
        if (fold) { e.obs_of_next = c.env->obs; e.nc = f.nc; e.noise = f.noise; e.obs_epoch = epoch + 1; e.obs_epoch_base = epoch_base; }
        return rq::launch_step(c.dev->stream, e);
    }
    rq_env::GraphKey graph_key(const RolloutCall& c, const RolloutFrame& f) const {
        rq_env::GraphKey key;
        key.params = c.params->d; key.state = c.state->d; key.hidden = policy->hidden; key.packed = packed_of(policy);
        key.weights = policy->w_dev; key.obs = c.env->obs; key.flags = c.flags; key.precision = policy->precision; key.cfg = c.env->cfg;
        key.seed = c.rng->seed; key.sas_mode = policy->sas_mode; key.sas_seed = policy->sas_seed; key.ls_image = policy->ls_image;
        key.ref = f.trk.ref; key.ref_rows = f.trk.rows; key.row0_at = f.trk.row0_at;
        key.row0_gen = f.row0_gen;      // (a reference bank: which ids the rows were built from)
        key.interval = policy->native_interval;
        for (int k = 0; k < kScheduleKinds; ++k) key.schedule_gen[k] = c.env->schedule[k].gen;
        return key;
    }
};

// The tables of rq_reference_create (one table, named without a bank's words), rq_reference_bank_create and the three schedule
// banks: refused before the device is looked at, then allocated and uploaded.  T: the handle's type; `kind`: its row of kTableKinds.
template <typename T>
int row_tables_create(const char* who, int kind, rq_device* dev, const float* host_rows, uint32_t n_tables, uint32_t rows, T** out) {
    const TableKind& tk = kTableKinds[kind];
    const bool single = kind == kReference, names_column = tk.rule != TableKind::kFinite;
    const uint32_t cols = tk.cols;
    const std::string noun = tk.tables;
    RQ_REFUSE(who, dev && host_rows && out, RQ_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (single) RQ_REFUSE(who, rows > 0, RQ_ERR_INVALID_ARGUMENT, "a reference needs at least one row");
    RQ_REFUSE(who, n_tables > 0 && rows > 0, RQ_ERR_INVALID_ARGUMENT, "a " + noun + " needs at least one table of at least one row");
    // the row an env reads, first row of its table + episode step count, is a uint32 on the device
    RQ_REFUSE(who, single || (uint64_t)n_tables * rows < (1ull << 28), RQ_ERR_INVALID_ARGUMENT, "a " + noun + " holds fewer than 2^28 rows in all");
    const size_t floats = (size_t)n_tables * rows * cols;
    for (size_t j = 0; j < floats; ++j) {
        const char* bad = !std::isfinite(host_rows[j])                                                     ? " holds a non-finite entry"
                          : tk.rule == TableKind::kPositive && !(host_rows[j] > 0.0f)                       ? " holds a factor that is not > 0"
                          : tk.rule == TableKind::kNonNegativeColumn && (int)(j % cols) == tk.rule_col && !(host_rows[j] >= 0.0f)
                              ? " holds a negative drag"
                              : nullptr;
        RQ_REFUSE(who, !bad, RQ_ERR_INVALID_ARGUMENT,
                  noun + bad + (single ? "" : ": table " + std::to_string(j / ((size_t)rows * cols)) + ", row " + std::to_string(j / cols % rows)) +
                      (names_column ? ", column " + std::to_string(j % cols) : ""));
    }
    DeviceScope on_device(dev); int rc = on_device.rc; if (rc) return rc;
    T* r = new (std::nothrow) T();
    RQ_REFUSE(who, r, RQ_ERR_OUT_OF_MEMORY, "host allocation failed");
    r->dev = dev; r->ordinal = dev->ordinal; r->n_tables = n_tables; r->rows = rows;
    if (r->d.alloc(floats) != hipSuccess) {
        delete r;
        return fail(RQ_ERR_OUT_OF_MEMORY, std::string(who) + ": device allocation failed");
    }
    // (synchronous: the caller's rows are its own again on return)
    const hipError_t e = hipMemcpy(r->d, host_rows, floats * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        delete r;
        return hip_failed(who, "hipMemcpy", e);
    }
    *out = r;
    return RQ_OK;
}

// the handles die alike: on their device, where hipFree synchronises (no launch still reads the tables)
template <typename T>
int row_tables_destroy(T* tables) {
    if (!tables) return RQ_OK;
    DeviceScope on_device(tables->ordinal);
    delete tables;
    return RQ_OK;
}


// ---- the schedules' entry points, one body per verb; `kind`: the schedule's row of kTableKinds ----
int schedule_bank_destroy(const char* who, int kind, ScheduleBank* bank) {
    const TableKind& tk = kTableKinds[kind];
    RQ_REFUSE(who, !bank || bank->attached == 0, RQ_ERR_INVALID_ARGUMENT,
              std::string("the ") + tk.tables + " is attached to " + std::to_string(bank->attached) + " live env(s): detach it (" + tk.detach +
                  " with a NULL bank) or destroy the env first");
    return RQ_OK;
}

// attach `bank` with one id per env (null: table 0 for all), or detach (null bank)
int env_schedule_set(const char* who, int kind, rq_env* env, ScheduleBank* bank, const uint32_t* id) {
    const std::string noun = kTableKinds[kind].noun;
    RQ_REFUSE(who, env, RQ_ERR_INVALID_ARGUMENT, "null argument");
    rq_device* dev = env->dev;
    if (bank) {
        RQ_REFUSE(who, bank->dev == dev, RQ_ERR_SHAPE_MISMATCH, noun + " bank lives on another device");
        for (uint32_t i = 0; id && i < env->n; ++i)
            RQ_REFUSE(who, id[i] < bank->n_tables, RQ_ERR_INVALID_ARGUMENT,
                      noun + " id out of range: env " + std::to_string(i) + " names table " + std::to_string(id[i]) + " of a bank of " +
                          std::to_string(bank->n_tables));
    }
    DeviceScope on_device(dev); int rc = on_device.rc; if (rc) return rc;      // (retires a running resident executor)
    RQ_HIP_AS(who, hipStreamSynchronize(dev->stream));        // a launch in flight reads the rows of the schedule before
    obs_cache_drop_if(dev, env);
    auto& slot = env->schedule[kind];
    if (!bank) { slot.detach(); return RQ_OK; }
    if (kind == kDelay)      // with the env's command history: made on the first attachment, zeroed at every one
        return first_rows_failed("delay schedule", env->delay_history.attach(dev->stream, slot, bank, id, env->n, env->ld,
                                                                             (size_t)rq::kDelaySlots * RQ_ACTION_DIM * env->ld));
    if (kind == kSensor)     // with the env's readings: likewise, a ring of its own
        return first_rows_failed("sensor schedule", env->sensor_history.attach(dev->stream, slot, bank, id, env->n, env->ld,
                                                                              (size_t)rq::kSensorSlots * rq::kSensorFields * env->ld));
    return first_rows_failed((noun + " schedule").c_str(), slot.attach(dev->stream, bank, id, env->n, env->ld));
}

template <typename T>
int env_schedule_get(const char* who, int kind, const rq_env* env, T** bank, uint32_t* id_out) {
    RQ_REFUSE(who, env && bank, RQ_ERR_INVALID_ARGUMENT, "null argument");
    const auto& slot = env->schedule[kind];
    *bank = static_cast<T*>(slot.bank);
    if (slot.bank && id_out) std::memcpy(id_out, slot.ids.data(), (size_t)env->n * sizeof(uint32_t));
    return RQ_OK;
}

// a delay bank's and a sensor bank's entries are bytes: their own checks, in the words of row_tables_create, then the same handle
// (`noun`: "delay", "sensor"; `max_steps`: RQ_DELAY_MAX_STEPS, RQ_SENSOR_MAX_STEPS)
template <typename T>
int steps_bank_create(const char* who, const std::string& noun, uint32_t max_steps, rq_device* dev, const uint8_t* host_rows,
                             uint32_t n_tables, uint32_t rows, T** out) {
    RQ_REFUSE(who, dev && host_rows && out, RQ_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    RQ_REFUSE(who, n_tables > 0 && rows > 0, RQ_ERR_INVALID_ARGUMENT, "a " + noun + " bank needs at least one table of at least one row");
    RQ_REFUSE(who, (uint64_t)n_tables * rows < (1ull << 28), RQ_ERR_INVALID_ARGUMENT, "a " + noun + " bank holds fewer than 2^28 rows in all");
    const size_t bytes = (size_t)n_tables * rows;
    for (size_t j = 0; j < bytes; ++j)
        RQ_REFUSE(who, host_rows[j] <= max_steps, RQ_ERR_INVALID_ARGUMENT,
                  noun + " bank holds a delay above " + std::to_string(max_steps) + " steps: table " + std::to_string(j / rows) +
                      ", row " + std::to_string(j % rows) + " (" + std::to_string((unsigned)host_rows[j]) + ")");
    DeviceScope on_device(dev); int rc = on_device.rc; if (rc) return rc;
    T* r = new (std::nothrow) T();
    RQ_REFUSE(who, r, RQ_ERR_OUT_OF_MEMORY, "host allocation failed");
    r->dev = dev; r->ordinal = dev->ordinal; r->n_tables = n_tables; r->rows = rows;
    if (r->steps.alloc(bytes) != hipSuccess) {
        delete r;
        return fail(RQ_ERR_OUT_OF_MEMORY, std::string(who) + ": device allocation failed");
    }
    const hipError_t e = hipMemcpy(r->steps, host_rows, bytes, hipMemcpyHostToDevice);      // (synchronous, as row_tables_create's)
    if (e != hipSuccess) {
        delete r;
        return hip_failed(who, "hipMemcpy", e);
    }
    *out = r;
    return RQ_OK;
}
}  // namespace

extern "C" {

RQ_API int rq_rollout(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state, rq_policy* policy,
               rq_rng* rng, uint32_t n_steps, int mode, uint32_t flags) {
    return rollout_run({__func__, dev, env, params, state, rng, n_steps, mode, flags, nullptr, nullptr, nullptr}, PolicyActor{policy});
}

RQ_API int rq_rollout_record(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state, rq_policy* policy,
                      rq_rng* rng, uint32_t n_steps, int mode, uint32_t flags, rq_trajectory* trajectory) {
    RQ_REQUIRE(trajectory, RQ_ERR_INVALID_ARGUMENT, "null trajectory");
    return rollout_run({__func__, dev, env, params, state, rng, n_steps, mode, flags, trajectory, nullptr, nullptr}, PolicyActor{policy});
}

RQ_API int rq_rollout_track(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state, rq_policy* policy,
                     rq_rng* rng, uint32_t n_steps, int mode, uint32_t flags, rq_trajectory* trajectory,
                     const rq_reference* reference) {
    RQ_REQUIRE(reference, RQ_ERR_INVALID_ARGUMENT, "null reference");
    return rollout_run({__func__, dev, env, params, state, rng, n_steps, mode, flags, trajectory, reference, nullptr}, PolicyActor{policy});
}

RQ_API int rq_rollout_track_refs(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state, rq_policy* policy,
                                 rq_rng* rng, uint32_t n_steps, int mode, uint32_t flags, rq_trajectory* trajectory,
                                 const rq_reference_bank* references, const uint32_t* reference_id) {
    RQ_REQUIRE(references, RQ_ERR_INVALID_ARGUMENT, "null reference bank");
    RQ_REQUIRE(reference_id, RQ_ERR_INVALID_ARGUMENT, "null reference_id");
    return rollout_run({__func__, dev, env, params, state, rng, n_steps, mode, flags, trajectory, references, reference_id},
                       PolicyActor{policy});
}

// ---------------------------------------------------------------------------- Tracking
RQ_API int rq_reference_create(rq_device* dev, const float* host_rows, uint32_t rows, rq_reference** out) {
    return row_tables_create(__func__, kReference, dev, host_rows, 1, rows, out);
}

RQ_API int rq_reference_destroy(rq_reference* reference) { return row_tables_destroy(reference); }

RQ_API int rq_reference_bank_create(rq_device* dev, const float* host_rows, uint32_t n_refs, uint32_t rows, rq_reference_bank** out) {
    return row_tables_create(__func__, kReferenceBank, dev, host_rows, n_refs, rows, out);
}

RQ_API int rq_reference_bank_destroy(rq_reference_bank* references) { return row_tables_destroy(references); }

// ---------------------------------------------------------------------------- Schedules: wrench, vehicle, wind, delay, sensor
RQ_API int rq_wrench_bank_create(rq_device* dev, const float* host_rows, uint32_t n_tables, uint32_t rows, int units, rq_wrench_bank** out) {
    RQ_REQUIRE(units == RQ_WRENCH_RELATIVE || units == RQ_WRENCH_ABSOLUTE, RQ_ERR_INVALID_ARGUMENT,
               "unknown units: RQ_WRENCH_RELATIVE or RQ_WRENCH_ABSOLUTE");
    const int rc = row_tables_create(__func__, kWrench, dev, host_rows, n_tables, rows, out);
    if (rc == RQ_OK) (*out)->units = units;
    return rc;
}
RQ_API int rq_vehicle_bank_create(rq_device* dev, const float* host_rows, uint32_t n_tables, uint32_t rows, rq_vehicle_bank** out) {
    return row_tables_create(__func__, kVehicle, dev, host_rows, n_tables, rows, out);
}
RQ_API int rq_wind_bank_create(rq_device* dev, const float* host_rows, uint32_t n_tables, uint32_t rows, rq_wind_bank** out) {
    return row_tables_create(__func__, kWind, dev, host_rows, n_tables, rows, out);
}

RQ_API int rq_delay_bank_create(rq_device* dev, const uint8_t* host_rows, uint32_t n_tables, uint32_t rows, rq_delay_bank** out) {
    return steps_bank_create(__func__, "delay", RQ_DELAY_MAX_STEPS, dev, host_rows, n_tables, rows, out);
}
RQ_API int rq_sensor_bank_create(rq_device* dev, const uint8_t* host_rows, uint32_t n_tables, uint32_t rows, rq_sensor_bank** out) {
    return steps_bank_create(__func__, "sensor", RQ_SENSOR_MAX_STEPS, dev, host_rows, n_tables, rows, out);
}

RQ_API int rq_wrench_bank_destroy(rq_wrench_bank* bank) {
    const int rc = schedule_bank_destroy(__func__, kWrench, bank);
    return rc ? rc : row_tables_destroy(bank);
}
RQ_API int rq_vehicle_bank_destroy(rq_vehicle_bank* bank) {
    const int rc = schedule_bank_destroy(__func__, kVehicle, bank);
    return rc ? rc : row_tables_destroy(bank);
}
RQ_API int rq_wind_bank_destroy(rq_wind_bank* bank) {
    const int rc = schedule_bank_destroy(__func__, kWind, bank);
    return rc ? rc : row_tables_destroy(bank);
}

RQ_API int rq_delay_bank_destroy(rq_delay_bank* bank) {
    const int rc = schedule_bank_destroy(__func__, kDelay, bank);
    return rc ? rc : row_tables_destroy(bank);
}

RQ_API int rq_sensor_bank_destroy(rq_sensor_bank* bank) {
    const int rc = schedule_bank_destroy(__func__, kSensor, bank);
    return rc ? rc : row_tables_destroy(bank);
}

RQ_API int rq_env_set_wrench_schedule(rq_env* env, rq_wrench_bank* bank, const uint32_t* wrench_id) {
    return env_schedule_set(__func__, kWrench, env, bank, wrench_id);
}
RQ_API int rq_env_set_vehicle_schedule(rq_env* env, rq_vehicle_bank* bank, const uint32_t* vehicle_id) {
    return env_schedule_set(__func__, kVehicle, env, bank, vehicle_id);
}
RQ_API int rq_env_set_wind_schedule(rq_env* env, rq_wind_bank* bank, const uint32_t* wind_id) {
    return env_schedule_set(__func__, kWind, env, bank, wind_id);
}

RQ_API int rq_env_set_delay_schedule(rq_env* env, rq_delay_bank* bank, const uint32_t* delay_id) {
    return env_schedule_set(__func__, kDelay, env, bank, delay_id);
}
RQ_API int rq_env_clear_delay_schedule(rq_env* env) { return env_schedule_set(__func__, kDelay, env, nullptr, nullptr); }

RQ_API int rq_env_set_sensor_schedule(rq_env* env, rq_sensor_bank* bank, const uint32_t* sensor_id) {
    return env_schedule_set(__func__, kSensor, env, bank, sensor_id);
}
RQ_API int rq_env_clear_sensor_schedule(rq_env* env) { return env_schedule_set(__func__, kSensor, env, nullptr, nullptr); }

RQ_API int rq_env_get_wrench_schedule(const rq_env* env, rq_wrench_bank** bank, uint32_t* wrench_id_out) {
    return env_schedule_get(__func__, kWrench, env, bank, wrench_id_out);
}
RQ_API int rq_env_get_vehicle_schedule(const rq_env* env, rq_vehicle_bank** bank, uint32_t* vehicle_id_out) {
    return env_schedule_get(__func__, kVehicle, env, bank, vehicle_id_out);
}
RQ_API int rq_env_get_wind_schedule(const rq_env* env, rq_wind_bank** bank, uint32_t* wind_id_out) {
    return env_schedule_get(__func__, kWind, env, bank, wind_id_out);
}

RQ_API int rq_env_get_delay_schedule(const rq_env* env, rq_delay_bank** bank, uint32_t* delay_id_out) {
    return env_schedule_get(__func__, kDelay, env, bank, delay_id_out);
}

RQ_API int rq_env_get_sensor_schedule(const rq_env* env, rq_sensor_bank** bank, uint32_t* sensor_id_out) {
    return env_schedule_get(__func__, kSensor, env, bank, sensor_id_out);
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
