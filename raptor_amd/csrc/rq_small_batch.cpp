// rq_small_batch.cpp - the small-batch loop's mailbox, observation cache and speculative policy step (rq_device::mailbox / obs_cache / spec).
#include "rq_objects.hpp"

namespace rqh {

void small_batch_setup(rq_device* dev) { dev->spec.enabled = std::getenv("RQ_NO_SPECULATION") == nullptr; }

// ---- mailbox --------------------------------------------------------------------------------------------------------------------------
constexpr size_t kMailboxRowFloats = (size_t)(kGpuLayoutMinEnvs - 1) * 32;

int ensure_mailbox(rq_device* dev) {
    HostMailbox& m = dev->mailbox;
    if (m.flag) return RQ_OK;
    RQ_HIP(m.flag.alloc(16));
    *static_cast<volatile uint32_t*>(m.flag.get()) = 0;
    hipError_t e = m.in.alloc(kMailboxRowFloats);
    if (e == hipSuccess) e = m.out.alloc(kMailboxRowFloats);
    if (e == hipSuccess) e = m.counter.alloc(1);
    if (e == hipSuccess) e = hipMemsetAsync(m.counter, 0, sizeof(uint32_t), dev->stream);
    if (e == hipSuccess) e = m.obs.alloc(kMailboxRowFloats);
    if (e == hipSuccess) e = m.act.alloc((size_t)kGpuLayoutMinEnvs * RQ_ACTION_DIM);
    if (e != hipSuccess) { m = HostMailbox{}; return fail(RQ_ERR_OUT_OF_MEMORY, "ensure_mailbox: pinned host allocation failed"); }
    return RQ_OK;
}

// spin until the launch with sequence number seq (or a later one: launches finish in stream order) signalled.  While the
// resident executor runs, the work waited for may be a command posted to it: if it has left (`exited`) without consuming the
// command, resident_gone() replays the command as launches on the stream and the wait goes on.
int mailbox_wait(rq_device* dev, uint32_t seq) {
    const ResidentExecutor& rx = dev->resident;
    for (uint64_t spins = 1;; ++spins) {
        const uint32_t f = __atomic_load_n(dev->mailbox.flag.get(), __ATOMIC_ACQUIRE);
        if ((int32_t)(f - seq) >= 0) return RQ_OK;
        if (rx.running && (spins & 0xFFu) == 0 && resident_left(dev)) {
            const int rc = resident_gone(dev); if (rc) return rc;
            continue;
        }
        if ((spins & 0xFFFFu) == 0) {           // every ~100 us: is the stream still alive?
            const hipError_t q = hipStreamQuery(rx.running ? rx.stream : dev->stream);
            if (q == hipSuccess) {
                if (rx.running) { const int rc = resident_gone(dev); if (rc) return rc; continue; }
                const uint32_t g = __atomic_load_n(dev->mailbox.flag.get(), __ATOMIC_ACQUIRE);
                if ((int32_t)(g - seq) >= 0) return RQ_OK;
                return fail(RQ_ERR_HIP, "mailbox_wait: the stream drained without the kernel signalling");
            }
            if (q != hipErrorNotReady) RQ_HIP(q);
        }
        __builtin_ia32_pause();
    }
}

// once the launch with sequence number seq has signalled: `floats` floats of the pinned rows it wrote into dst
int mailbox_copy_out(rq_device* dev, uint32_t seq, const float* rows, float* dst, size_t floats) {
    const int rc = mailbox_wait(dev, seq); if (rc) return rc;
    std::memcpy(dst, rows, floats * sizeof(float));
    return RQ_OK;
}

// n host rows of dim floats at `stride` into `in`, once the last launch reading it has finished
int mailbox_put_in(rq_device* dev, const float* rows, uint32_t n, uint32_t dim, size_t stride) {
    HostMailbox& m = dev->mailbox;
    if (m.in_busy) { const int rc = mailbox_wait(dev, m.in_busy); if (rc) return rc; m.in_busy = 0; }
    if (stride == dim) std::memcpy(m.in, rows, (size_t)n * dim * sizeof(float));
    else for (uint32_t i = 0; i < n; ++i) std::memcpy(m.in + (size_t)i * dim, rows + (size_t)i * stride, dim * sizeof(float));
    return RQ_OK;
}

rq::Mailbox mailbox_for(rq_device* dev, bool reads_in, uint32_t in_stride, MbOut out) {
    HostMailbox& m = dev->mailbox;
    rq::Mailbox mb{};
    mb.rows_in = reads_in ? m.in : nullptr; mb.in_stride = in_stride;
    mb.rows_out = out == MbOut::out ? m.out : out == MbOut::obs ? m.obs : out == MbOut::act ? m.act : nullptr;
    mb.counter = m.counter; mb.flag = m.flag;
    if (++m.seq == 0) ++m.seq;      // 0 means "nothing pending"
    mb.seq = m.seq;
    if (reads_in) m.in_busy = mb.seq;
    return mb;
}

// the mailbox of a small-batch step: host actions into `in` (the kernel files them in env->act), the observation into the cache's rows
int mailbox_for_step(rq_device* dev, const float* action, uint32_t n, bool cache_obs, rq::Mailbox* mb) {
    int rc = ensure_mailbox(dev); if (rc) return rc;
    if (action) { rc = mailbox_put_in(dev, action, n, RQ_ACTION_DIM, RQ_ACTION_DIM); if (rc) return rc; }
    // about to be rewritten: no host reader of the cached rows can exist (calls are synchronous), but their producer must be done
    if (cache_obs && dev->obs_cache.env) { rc = mailbox_wait(dev, dev->obs_cache.seq); if (rc) return rc; }
    *mb = mailbox_for(dev, action != nullptr, RQ_ACTION_DIM, cache_obs ? MbOut::obs : MbOut::none);
    return RQ_OK;
}

// a launch that was handed a mailbox failed: nothing will ever publish its sequence number
void mailbox_abort(rq_device* dev, const rq::Mailbox& mb) {
    HostMailbox& m = dev->mailbox;
    if (mb.flag == nullptr) return;
    if (m.in_busy == mb.seq) m.in_busy = 0;
    if (m.seq == mb.seq) m.seq = mb.seq - 1;      // 0 ("nothing pending") is skipped by mailbox_for
}

// the pinned rows a resident kernel reads and writes as the launches it stands for would, and the flag it publishes in
void mailbox_resident_args(const rq_device* dev, rq::ResidentArgs& ra, bool policy_kind) {
    const HostMailbox& m = dev->mailbox;
    ra.flag = m.flag; ra.rows_act = policy_kind ? m.out : m.act;
    if (!policy_kind) { ra.rows_action = m.in; ra.rows_obs = m.obs; }
}

// ---- observation cache ----------------------------------------------------------------------------------------------------------------
bool obs_cache_holds(const rq_device* dev, const rq_env* env, const rq_params* params, const rq_state* state) {
    const ObservationCache& oc = dev->obs_cache;
    if (oc.env != env || oc.env_uid != env->uid || env->obs_exposed || oc.params != params || params->exposed ||
        params->version != oc.params_version || state->exposed)
        return false;
    return (oc.state[0] == state && oc.version[0] == state->version) || (oc.state[1] == state && oc.version[1] == state->version);
}

// a hit: obs_alt holds the observation on the device (swapped in here), the cache's rows for the host (once its launch's flag is set)
int obs_cache_read(rq_device* dev, rq_env* env, float* observation) {
    ObservationCache& oc = dev->obs_cache;
    if (oc.in_alt) { env->obs.swap(env->obs_alt); oc.in_alt = false; }
    return observation ? mailbox_copy_out(dev, oc.seq, dev->mailbox.obs, observation, (size_t)env->n * RQ_OBSERVATION_DIM) : RQ_OK;
}

void obs_cache_drop(rq_device* dev) { dev->obs_cache.env = nullptr; dev->obs_cache.state[0] = dev->obs_cache.state[1] = nullptr; }

// a real observation of env, or its state stepped on the device, replaces what was cached for it
void obs_cache_drop_if(rq_device* dev, const rq_env* env) { if (dev->obs_cache.env == env) obs_cache_drop(dev); }

// the step that wrote `state` (mailbox sequence number seq) fills the cache's rows, and pol (or nullptr) was speculated on them, its
// actions published as spec_seq: the one speculation a later evaluate_step may take
void obs_cache_fill(rq_device* dev, const rq_env* env, const rq_params* params, const rq_state* state, uint32_t seq, rq_policy* pol, uint32_t spec_seq) {
    ObservationCache& oc = dev->obs_cache;
    oc.env = env; oc.env_uid = env->uid; oc.params = params; oc.params_version = params->version;
    oc.state[0] = state; oc.version[0] = state->version; oc.state[1] = nullptr;
    oc.seq = seq; oc.n = env->n; oc.in_alt = true;
    Speculation& sp = dev->spec; sp.policy = pol;
    if (pol) { sp.policy_version = pol->version; sp.batch = env->n; sp.seq = spec_seq; sp.oc_seq = seq; sp.outstanding = true; }
}

// state.assign(src): the cached observation of src is the observation of dst now
void obs_cache_follow_assign(rq_device* dev, const rq_state* dst, const rq_state* src) {
    ObservationCache& oc = dev->obs_cache;
    if (oc.state[0] == src && oc.version[0] == src->version && !src->exposed) { oc.state[1] = dst; oc.version[1] = dst->version; }
}

static bool rows_match(const rq_device* dev, const float* rows, uint32_t n, uint32_t stride) {
    for (uint32_t i = 0; i < n; ++i)
        if (std::memcmp(rows + (size_t)i * stride, dev->mailbox.obs + (size_t)i * RQ_OBSERVATION_DIM, RQ_POLICY_INPUT_DIM * sizeof(float)))
            return false;
    return true;
}

// ---- speculative policy step ----------------------------------------------------------------------------------------------------------
static bool speculation_current(const rq_device* dev) { return dev->obs_cache.env && dev->spec.oc_seq == dev->obs_cache.seq; }

// a speculated policy step that was launched is about to be superseded or was passed over: count it
static void speculation_unused(rq_device* dev) {
    Speculation& sp = dev->spec;
    if (sp.outstanding && ++sp.misses >= kSpeculationMissLimit) sp.suspended = true;
    sp.outstanding = false;
}

// the policy a step of env (cache_obs: its observation will be cached; action: host actions) speculates with, or nullptr
rq_policy* speculation_candidate(rq_device* dev, const rq_env* env, bool cache_obs, bool action) {
    if (!cache_obs) return nullptr;
    speculation_unused(dev);      // the previous step's speculated policy step, if nobody took it (this may suspend speculation)
    const Speculation& sp = dev->spec;
    // (an env that carries a schedule is stepped by plain launches: neither speculated on nor handed to the resident executor)
    rq_policy* pol = sp.enabled && !sp.suspended && action && !env->has_schedule() ? sp.last_policy : nullptr;
    return pol && policy_registry(pol, 0) && pol->dev == dev && pol->batch == env->n && pol->ld == env->ld && pol->hidden &&
           pol->hidden_alt && !pol->needs_reset && pol->sas_mode != RQ_SAS_SAMPLE && pol->native_interval == 1 ? pol : nullptr;
}

// evaluate_step of pol on host rows, before anything is launched.  *hit: rq_step speculated exactly this call, `action` holds the result.
// Otherwise the call is recorded: a miss, the end of a suspension, the policy the next step speculates with.
int speculation_take(rq_device* dev, rq_policy* pol, const float* observation, uint32_t batch, uint32_t obs_stride, float* action, bool* hit) {
    Speculation& sp = dev->spec; const ObservationCache& oc = dev->obs_cache;
    *hit = false;
    if (sp.policy == pol && sp.policy_version == pol->version && sp.batch == batch && speculation_current(dev) &&
        mailbox_wait(dev, oc.seq) == RQ_OK && rows_match(dev, observation, batch, obs_stride)) {
        const int rc = mailbox_copy_out(dev, sp.seq, dev->mailbox.act, action, (size_t)batch * RQ_ACTION_DIM); if (rc) return rc;
        pol->hidden.swap(pol->hidden_alt);             // the speculated step becomes the policy's state
        pol->version = fresh_version();
        sp.policy = nullptr; sp.last_policy = pol; sp.outstanding = false; sp.misses = 0;
        *hit = true; return RQ_OK;
    }
    // a speculated step of THIS policy that did not match is spent; ANOTHER policy's stays available - it depends on that policy's version
    // and the cached rows only (a loop evaluating a student and a teacher on the same rows would otherwise throw the teacher's step away)
    if (sp.policy == pol) { speculation_unused(dev); sp.policy = nullptr; }
    // suspended after a run of misses: a call that is what a hit would have been means the loop is back in the reference's shape
    if (sp.suspended && sp.enabled && sp.last_policy == pol && oc.env && batch == oc.n && mailbox_wait(dev, oc.seq) == RQ_OK &&
        rows_match(dev, observation, batch, obs_stride)) { sp.suspended = false; sp.misses = 0; }
    sp.last_policy = pol;         // the policy rq_step will speculate with
    return RQ_OK;
}

// the two launches of a small-batch step on the device's stream (also the replay of a command the resident executor never consumed)
hipError_t launch_step_pair(rq_device* dev, const StepPair& p) {
    hipError_t e = rq::launch_step(dev->stream, p.step);
    if (e == hipSuccess && p.spec) e = rq::launch_actor_step(dev->stream, p.actor);
    return e;
}

}  // namespace rqh

using namespace rqh;

extern "C" {

RQ_API int rq_device_set_speculation(rq_device* dev, int enable) {
    RQ_REQUIRE(dev, RQ_ERR_INVALID_ARGUMENT, "null argument");
    Speculation& sp = dev->spec;
    sp.enabled = enable != 0; sp.suspended = false; sp.misses = 0;
    if (!sp.enabled) { sp.policy = nullptr; sp.outstanding = false; }
    return RQ_OK;
}

RQ_API int rq_device_get_speculation(const rq_device* dev, int* enabled, int* suspended, uint32_t* consecutive_misses) {
    RQ_REQUIRE(dev, RQ_ERR_INVALID_ARGUMENT, "null argument");
    if (enabled) *enabled = dev->spec.enabled ? 1 : 0;
    if (suspended) *suspended = dev->spec.suspended ? 1 : 0;
    if (consecutive_misses) *consecutive_misses = dev->spec.misses;
    return RQ_OK;
}

}  // extern "C"
