// rq_capi_grad.cpp - the learner half of distillation (README.md:208-216) behind the C ABI: the fp32 student over a recorded
// trajectory (rq_trajectory_policy_forward) and the exact gradient of those actions with respect to its 2 084 parameters, back
// through time along the recorded episode structure (rq_trajectory_policy_backward); and the whole distillation update on the device:
// masked-MSE loss and gradient (rq_trajectory_policy_loss_grad), Adam and the operand images (rq_trajectory_distill); and that update
// for every policy of a policy bank at once (rq_trajectory_policies_loss_grad, rq_bank_optimizer_*, rq_trajectory_policies_distill).
// Adam's state as host arrays and one update from the caller's gradient - what checkpoints a run and what tests the update kernel on
// arbitrary inputs (rq_optimizer_get_state / _set_state / _apply, rq_bank_optimizer_get_state / _set_state).
// The four loss calls have a *_weighted sibling each - a weight per env, or per env and step, in the loss - that shares their body.
// rq_trajectory_policy_error_table / rq_trajectory_policies_error_table: the forward alone against the loss calls' target - the
// squared imitation error per env and bucket of episode age; the trajectory's saved state is not theirs and stays as it was.
// rq_trajectory_policy_gain_table / rq_trajectory_policies_gain_table: A = da/dp0 summed per env and bucket of episode age, the
// effective feedback gains up to the constant W0; no target, the saved state stays as it was too.
// Every call with a `memory` argument reads refusals, DeviceScope, prepare, in, launch, out, finish: the staging copies and the final
// wait are one rq::CallMemory (rq_call_memory.hpp), the staging buffers are reserved here.  Kernels: rq_grad.hpp, rq_grad_bank.hpp.
#include "rq_objects.hpp"

#include <cfloat>

using namespace rqh;

namespace rqh {

// what both directions refuse: only the fp32 student without input or output stages has a gradient here
int grad_check_pair(rq_trajectory* t, rq_policy* pol, const char* what) {
    RQ_REQUIRE(t && pol, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(pol->dev == t->env->dev, RQ_ERR_SHAPE_MISMATCH, std::string(what) + ": the policy lives on another device");
    RQ_REQUIRE(t->length > 0, RQ_ERR_INVALID_ARGUMENT, std::string(what) + ": the trajectory is empty");
    RQ_REQUIRE(pol->precision == RQ_POLICY_FP32, RQ_ERR_INVALID_ARGUMENT,
               std::string(what) + ": defined for the fp32 policy only (set_precision(RQ_POLICY_FP32)), not bf16 or f16x2");
    RQ_REQUIRE(!pol->standardize, RQ_ERR_INVALID_ARGUMENT,
               std::string(what) + ": the Standardize stage has no gradient here (disable it)");
    RQ_REQUIRE(pol->sas_mode == RQ_SAS_OFF, RQ_ERR_INVALID_ARGUMENT,
               std::string(what) + ": the SampleAndSquash stage has no gradient here (RQ_SAS_OFF)");
    return require_native_rate(pol, what);
}

int grad_saved_initial(rq_trajectory* t, rq_policy* pol) {
    rq_env* env = t->env; rq_device* dev = env->dev;
    if (t->grad.matches(pol, t->length) && t->grad.weight_version == pol->weight_version && t->grad.start == RQ_GRAD_START_INITIAL)
        return RQ_OK;
    t->grad.valid = false;
    RQ_HIP(t->grad.saved.reserve(dev->stream, (size_t)t->length * RQ_POLICY_HIDDEN_DIM * env->ld));
    rq::LossLaunch a;
    a.n = env->n; a.ld = env->ld; a.steps = t->length;
    a.packed = pol->w_packed; a.obs = t->obs; a.done = t->done;
    a.ld_h = pol->ld; a.start_initial = true; a.saved = t->grad.saved;
    RQ_HIP(rq::launch_policy_grad_forward_state(dev->stream, a));
    t->grad.stamp(pol, t->length, RQ_GRAD_START_INITIAL);
    return RQ_OK;
}

int check_memory(int memory) {
    RQ_REQUIRE(CallMemory::valid(memory), RQ_ERR_INVALID_ARGUMENT, "memory must be 0, 1 or 2");
    return RQ_OK;
}

int check_device_array(const CallMemory& mem, const void* p, const char* what, const char* noun) {
    RQ_REQUIRE(mem.host() || mem.on_device(p), RQ_ERR_SHAPE_MISMATCH,
               std::string(what) + ": " + noun + " lives on another device (or on the host): device memory of the trajectory's device is expected");
    return RQ_OK;
}

}  // namespace rqh

namespace {

// the transposed image of the backward, packed once per weight version (a device-side update writes it itself)
int ensure_grad_image(rq_policy* pol) {
    if (pol->w_packed_grad && pol->grad_image_version == pol->weight_version) return RQ_OK;
    rq_device* dev = pol->dev;
    int rc = policy_mirror(pol); if (rc) return rc;
    std::vector<float> image;
    try { image.resize(rq::RQ_PACKED_GRAD_FLOATS); } catch (const std::bad_alloc&) {
        return fail(RQ_ERR_OUT_OF_MEMORY, "rq_trajectory_policy_forward: host allocation failed");
    }
    rq::pack_policy_grad(pol->w_eff, image.data());
    RQ_HIP(hipStreamSynchronize(dev->stream));
    RQ_HIP(pol->w_packed_grad.reserve(dev->stream, image.size()));
    RQ_HIP(hipMemcpy(pol->w_packed_grad, image.data(), image.size() * sizeof(float), hipMemcpyHostToDevice));
    pol->grad_image_version = pol->weight_version;
    return RQ_OK;
}

// What the two loss-seeded calls share.  loss_check: the refusals, before the call's DeviceScope (a refused call leaves the device,
// a resident executor included, alone).  loss_begin, inside it: the workspace and the target on the device; n_losses: floats wanted
// behind the gradient in t->grad.out.  -> the launch (rq::LossLaunch) but for `grad` and `loss`, which the call sets - an update loop
// per iteration - before it hands it to rq::launch_policy_loss_grad.  loss_check_call and loss_workspace are the parts
// that do not ask whose weights they are: the bank's calls below share them.
// The *_weighted calls are their siblings with a LossWeight that is `given`: the weight [steps][ld] as the caller named it.  It
// travels like the target - a host array is copied in behind the target's staging, a device array is used where it lies.
struct LossWeight { bool given; const float* w; uint32_t ld, steps; };
constexpr LossWeight kNoWeight{false, nullptr, 0, 0};

int loss_check_call(rq_trajectory* t, const float* target, uint32_t ld_target, const LossWeight& wt, int start, int memory,
                    const char* what) {
    int rc = check_memory(memory); if (rc) return rc;
    RQ_REQUIRE(start == RQ_GRAD_START_CURRENT || start == RQ_GRAD_START_INITIAL, RQ_ERR_INVALID_ARGUMENT,
               "start must be RQ_GRAD_START_CURRENT or RQ_GRAD_START_INITIAL");
    const rq_device* dev = t->env->dev;
    const CallMemory mem(memory, dev->stream, dev->ordinal);
    const uint32_t n = t->env->n;
    if (target) {
        RQ_REQUIRE(ld_target >= n, RQ_ERR_INVALID_ARGUMENT, std::string(what) + ": ld_target must be at least the number of envs");
        rc = check_device_array(mem, target, what, "the target"); if (rc) return rc;
    }
    if (!wt.given) return RQ_OK;
    RQ_REQUIRE(wt.w, RQ_ERR_INVALID_ARGUMENT, std::string(what) + ": weight is null");
    RQ_REQUIRE(wt.steps == 1 || wt.steps == t->length, RQ_ERR_INVALID_ARGUMENT,
               std::string(what) + ": weight_steps must be 1 (a weight per env) or the trajectory's length " + std::to_string(t->length) +
                   " (one per env and step), not " + std::to_string(wt.steps));
    RQ_REQUIRE(wt.ld >= n, RQ_ERR_INVALID_ARGUMENT, std::string(what) + ": ld_weight must be at least the number of envs");
    if (!mem.host()) return check_device_array(mem, wt.w, what, "the weight");
    // a host array can be read here: a weight that cannot be meant is refused by name (on the device it is dropped, rq_grad_backward.inc)
    for (uint32_t s = 0; s < wt.steps; ++s)
        for (uint32_t i = 0; i < n; ++i) {
            const float w = wt.w[(size_t)s * wt.ld + i];
            RQ_REQUIRE(w >= 0.0f && w <= FLT_MAX, RQ_ERR_INVALID_ARGUMENT,
                       std::string(what) + ": weight of step " + std::to_string(s) + ", env " + std::to_string(i) +
                           " is negative or not finite (" + std::to_string(w) + ")");
        }
    return RQ_OK;
}

int loss_check(rq_trajectory* t, rq_policy* pol, const float* target, uint32_t ld_target, const LossWeight& wt, int start, int memory,
               const char* what) {
    int rc = grad_check_pair(t, pol, what); if (rc) return rc;
    return loss_check_call(t, target, ld_target, wt, start, memory, what);
}

// -> *a: the launch as far as it does not ask whose weights they are - the recording, the workspace reserved, the target and the
// weight on the device (staged through `mem`), the strides.  out_floats: what t->grad.out is to hold (gradients, then losses).
int loss_workspace(rq_trajectory* t, const float* target, uint32_t ld_target, const LossWeight& wt, int start, const CallMemory& mem,
                   size_t out_floats, rq::LossLaunch* a) {
    rq_env* env = t->env;
    rq_device* dev = env->dev;
    const uint32_t T = t->length, ld = env->ld;
    t->grad.valid = false;
    RQ_HIP(t->grad.saved.reserve(dev->stream, (size_t)T * RQ_POLICY_HIDDEN_DIM * ld));
    RQ_HIP(t->grad.partial.reserve(dev->stream, rq::loss_partial_layout(env->n, wt.given).floats));
    RQ_HIP(t->grad.out.reserve(dev->stream, out_floats));
    RQ_HIP(t->grad.live.reserve(dev->stream, 1));      // k_policy_loss_reduce stores M here; nobody reads it (the kernel's text stays)
    a->n = env->n; a->ld = ld; a->steps = T;
    a->obs = t->obs; a->done = t->done; a->saved = t->grad.saved;
    a->start_initial = start == RQ_GRAD_START_INITIAL;
    a->partial = t->grad.partial; a->live = t->grad.live;
    a->target = t->act.get();          // the stored actions: what a relabel or a teacher-acting rollout left
    a->ld_y = target ? ld_target : ld;
    // host-memory calls: one device block, the target | the weight, the second begun at a multiple of 256 bytes
    const size_t y_floats = target ? (size_t)T * RQ_ACTION_DIM * ld_target : 0, w_floats = wt.given ? (size_t)wt.steps * wt.ld : 0;
    const size_t off_w = wt.given ? (y_floats + 63) & ~(size_t)63 : y_floats;
    if (mem.host() && off_w + w_floats > 0) RQ_HIP(t->grad.rows.reserve(dev->stream, off_w + w_floats));
    if (target) RQ_HIP(mem.in(target, y_floats, t->grad.rows.get(), &a->target));
    if (wt.given) {
        RQ_HIP(mem.in(wt.w, w_floats, t->grad.rows.get() + off_w, &a->weight));
        a->ld_w = wt.ld; a->weight_steps = wt.steps;
    }
    return RQ_OK;
}

int loss_begin(rq_trajectory* t, rq_policy* pol, const float* target, uint32_t ld_target, const LossWeight& wt, int start,
               const CallMemory& mem, size_t n_losses, rq::LossLaunch* a) {
    int rc = RQ_OK;
    if (start == RQ_GRAD_START_CURRENT) { rc = policy_size(pol, t->env->n); if (rc) return rc; }
    rc = ensure_grad_image(pol); if (rc) return rc;
    rc = loss_workspace(t, target, ld_target, wt, start, mem, RQ_POLICY_NUM_WEIGHTS + n_losses, a); if (rc) return rc;
    a->packed = pol->w_packed; a->gpacked = pol->w_packed_grad;
    a->hidden = start == RQ_GRAD_START_CURRENT ? pol->hidden.get() : nullptr;
    a->ld_h = pol->ld;
    return RQ_OK;
}

// ---- the same for a policy bank (rq_trajectory_policies_loss_grad / _distill) ----
// bank_loss_check: every refusal, before the call's DeviceScope.  bank_loss_begin, inside it: the id table and the policies' wave
// lists (cached in the bank), the transposed images, for RQ_GRAD_START_CURRENT the bank's hidden state sized for this env and a
// pending reset applied - as rq_rollout_policies does -, then the workspace; n_losses: floats wanted behind the [P][2084]
// gradients in t->grad.out.
int bank_loss_check(rq_trajectory* t, rq_policy_bank* bank, const uint32_t* policy_id, const float* target, uint32_t ld_target,
                    const LossWeight& wt, int start, int memory, const char* what) {
    RQ_REQUIRE(bank->dev == t->env->dev, RQ_ERR_SHAPE_MISMATCH, std::string(what) + ": the policy bank lives on another device");
    RQ_REQUIRE(t->length > 0, RQ_ERR_INVALID_ARGUMENT, std::string(what) + ": the trajectory is empty");
    int rc = require_bank_native_rate(bank, what); if (rc) return rc;
    rc = loss_check_call(t, target, ld_target, wt, start, memory, what); if (rc) return rc;
    rc = bank_check_ids(bank, policy_id, t->env->n); if (rc) return rc;
    if (start == RQ_GRAD_START_CURRENT)
        RQ_REQUIRE(bank->batch == t->env->n || bank->batch == 0 || bank->needs_reset, RQ_ERR_SHAPE_MISMATCH,
                   std::string(what) + ": RQ_GRAD_START_CURRENT reads the bank's hidden state, which is sized for another batch");
    return RQ_OK;
}

int bank_loss_begin(rq_trajectory* t, rq_policy_bank* bank, const uint32_t* policy_id, const float* target, uint32_t ld_target,
                    const LossWeight& wt, int start, const CallMemory& mem, size_t n_losses, rq::LossLaunch* a) {
    rq_env* env = t->env;
    int rc = RQ_OK;
    if (start == RQ_GRAD_START_CURRENT) {
        rc = bank_size(bank, env->n); if (rc) return rc;
        RQ_REQUIRE(bank->ld == env->ld, RQ_ERR_SHAPE_MISMATCH, "policy bank batch does not match the env");
    }
    rc = bank_table(bank, env->dev, env->uid, policy_id, env->n); if (rc) return rc;
    rc = bank_wave_lists(bank); if (rc) return rc;
    rc = bank_grad_images(bank); if (rc) return rc;
    if (start == RQ_GRAD_START_CURRENT) { rc = bank_apply_reset(bank); if (rc) return rc; }
    rc = loss_workspace(t, target, ld_target, wt, start, mem, (size_t)bank->n_policies * RQ_POLICY_NUM_WEIGHTS + n_losses, a);
    if (rc) return rc;
    a->packed = bank->images; a->gpacked = bank->gimages;
    a->n_policies = bank->n_policies; a->block_policy = bank->table;
    a->wave_offsets = bank->waves; a->wave_list = bank->waves + bank->n_policies + 1;
    a->hidden = start == RQ_GRAD_START_CURRENT ? bank->hidden.get() : nullptr;
    a->ld_h = bank->ld;
    return RQ_OK;
}

// ---- the imitation error table (rq_trajectory_policy_error_table / rq_trajectory_policies_error_table) ----
// error_table_check: what the two calls refuse beyond their loss sibling's refusals (loss_check / bank_loss_check, which come first and
// have found `memory` valid), before the call's DeviceScope; -> the buckets in *a.  error_table_begin, inside it: the recording, the
// target and the outputs as the launch takes them.  The trajectory's saved state - t->grad.saved, its stamp - is not touched: the
// kernel stores nothing of the pass, and a rq_trajectory_policy_backward whose forward came before may follow.
// RQ_DST_HOST announces host arrays: device memory in their place is refused by name rather than handed to a host-to-device copy
int check_host_array(const CallMemory& mem, const void* p, const char* what, const char* noun) {
    if (!mem.host() || !p) return RQ_OK;
    hipPointerAttribute_t at{};
    const hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) (void)hipGetLastError();         // pageable memory the runtime has not seen: the query's error stays here
    RQ_REQUIRE(!(e == hipSuccess && at.type == hipMemoryTypeDevice), RQ_ERR_SHAPE_MISMATCH,
               std::string(what) + ": " + noun + " is device memory: RQ_DST_HOST expects a host array (RQ_DST_DEVICE takes device memory)");
    return RQ_OK;
}

// `Launch` is rq::ErrorTableLaunch or rq::GainTableLaunch (edges, n_buckets); `noun` names the float output, "sse" or "sum".
template <typename Launch>
int error_table_check(const char* what, rq_trajectory* t, const float* target, const uint32_t* age_edges, uint32_t n_buckets, float* sse,
                      uint32_t* count, uint32_t ld_out, int memory, Launch* a, const char* noun = "sse") {
    RQ_REFUSE(what, age_edges, RQ_ERR_INVALID_ARGUMENT, "null argument: age_edges");
    RQ_REFUSE(what, sse, RQ_ERR_INVALID_ARGUMENT, std::string("null argument: ") + noun);
    RQ_REFUSE(what, count, RQ_ERR_INVALID_ARGUMENT, "null argument: count");
    RQ_REFUSE(what, n_buckets >= 1 && n_buckets <= rq::kErrorTableMaxBuckets, RQ_ERR_INVALID_ARGUMENT,
              "n_buckets must be 1 .. 32, not " + std::to_string(n_buckets));
    for (uint32_t b = 0; b <= n_buckets; ++b) {
        RQ_REFUSE(what, b == 0 || age_edges[b] > age_edges[b - 1], RQ_ERR_INVALID_ARGUMENT,
                  "age_edges must ascend strictly (age_edges[" + std::to_string(b) + "] does not)");
        a->edges[b] = age_edges[b];
    }
    a->n_buckets = n_buckets;
    RQ_REFUSE(what, ld_out >= t->env->n, RQ_ERR_INVALID_ARGUMENT, "ld_out must be at least the number of envs");
    const rq_device* dev = t->env->dev;
    const CallMemory mem(memory, dev->stream, dev->ordinal);
    int rc = check_device_array(mem, sse, what, noun); if (rc) return rc;
    rc = check_device_array(mem, count, what, "count"); if (rc) return rc;
    rc = check_host_array(mem, target, what, "the target"); if (rc) return rc;
    rc = check_host_array(mem, sse, what, noun); if (rc) return rc;
    return check_host_array(mem, count, what, "count");
}

int error_table_begin(rq_trajectory* t, const float* target, uint32_t ld_target, int start, CallMemory& mem, float* sse, uint32_t* count,
                      uint32_t ld_out, rq::ErrorTableLaunch* a) {
    rq_env* env = t->env;
    rq_device* dev = env->dev;
    const uint32_t T = t->length, ld = env->ld, B = a->n_buckets;
    rq::LossLaunch& p = a->pass;
    p.n = env->n; p.ld = ld; p.steps = T;
    p.obs = t->obs; p.done = t->done;
    p.start_initial = start == RQ_GRAD_START_INITIAL;
    p.target = t->act.get();           // the stored actions: what a relabel or a teacher-acting rollout left
    p.ld_y = target ? ld_target : ld;
    // host-memory calls: one device block, sse [B][ld] | count [B][ld] | the target; only the envs' columns go back
    const size_t cells = (size_t)B * ld, y_floats = target ? (size_t)T * RQ_ACTION_DIM * ld_target : 0;
    float* s_sse = nullptr; uint32_t* s_count = nullptr;
    if (mem.host()) {
        RQ_HIP(t->grad.rows.reserve(dev->stream, 2 * cells + y_floats));
        s_sse = t->grad.rows.get();
        s_count = reinterpret_cast<uint32_t*>(s_sse + cells);
    }
    if (target) RQ_HIP(mem.in(target, y_floats, mem.host() ? s_sse + 2 * cells : nullptr, &p.target));
    a->sse = mem.out(sse, ld_out, s_sse, ld, env->n, B);
    a->count = mem.out(count, ld_out, s_count, ld, env->n, B);
    a->ld_out = mem.host() ? ld : ld_out;
    return RQ_OK;
}

// ---- the feedback-gain table (rq_trajectory_policy_gain_table / rq_trajectory_policies_gain_table) ----
// The error table's refusals (error_table_check, without a target) and its begin without one: sum [B][4][16][.] and count [B][.] as
// the launch takes them.  The saved state is not touched here either.
int gain_table_begin(rq_trajectory* t, int start, CallMemory& mem, float* sum, uint32_t* count, uint32_t ld_out, rq::GainTableLaunch* a) {
    rq_env* env = t->env;
    rq_device* dev = env->dev;
    const uint32_t ld = env->ld, B = a->n_buckets;
    rq::LossLaunch& p = a->pass;
    p.n = env->n; p.ld = ld; p.steps = t->length;
    p.obs = t->obs; p.done = t->done;
    p.start_initial = start == RQ_GRAD_START_INITIAL;
    // host-memory calls: one device block, sum [B][64][ld] | count [B][ld]; only the envs' columns go back
    const size_t rows = (size_t)B * RQ_ACTION_DIM * RQ_POLICY_HIDDEN_DIM, cells = rows * ld;
    float* s_sum = nullptr; uint32_t* s_count = nullptr;
    if (mem.host()) {
        RQ_HIP(t->grad.rows.reserve(dev->stream, cells + (size_t)B * ld));
        s_sum = t->grad.rows.get();
        s_count = reinterpret_cast<uint32_t*>(s_sum + cells);
    }
    a->sum = mem.out(sum, ld_out, s_sum, ld, env->n, rows);
    a->count = mem.out(count, ld_out, s_count, ld, env->n, B);
    a->ld_out = mem.host() ? ld : ld_out;
    return RQ_OK;
}

bool adam_config_ok(const rq_adam_config& c) {
    return c.lr >= 0.0 && c.eps >= 0.0 && c.weight_decay >= 0.0 && c.beta1 >= 0.0 && c.beta1 < 1.0 && c.beta2 >= 0.0 && c.beta2 < 1.0;
}

// Adam's state for `slots` policies, inside the caller's DeviceScope: moments zeroed, slot p's hyper-parameters from config[n_cfg == 1
// ? 0 : p], the repack's gather table.  zero_grad: the bank's gradient rows start at zero.  `who` begins the message of a failure.
int adam_alloc(const char* who, AdamBuffers* o, rq_device* dev, const rq_adam_config* config, uint32_t n_cfg, uint32_t slots,
               bool zero_grad) {
    o->dev = dev; o->ordinal = dev->ordinal;
    const size_t entries = (size_t)rq::RQ_PACKED_FLOATS + rq::RQ_PACKED_GRAD_FLOATS, floats = (size_t)slots * RQ_POLICY_NUM_WEIGHTS;
    std::vector<rq::PackGather> table;
    std::vector<rq::AdamState> st;
    try {
        table.resize(entries); rq::pack_gather_table(table.data());
        st.resize(slots);
    } catch (const std::bad_alloc&) {
        return fail(RQ_ERR_OUT_OF_MEMORY, std::string(who) + ": host allocation failed");
    }
    for (uint32_t p = 0; p < slots; ++p) {
        const rq_adam_config& c = config[n_cfg == 1 ? 0 : p];
        st[p] = rq::AdamState{c.lr, c.beta1, c.beta2, c.eps, c.weight_decay, 1.0, 1.0, 0u, 0u};
    }
    hipError_t e = o->m.alloc(floats);
    if (e == hipSuccess) e = o->v.alloc(floats);
    if (e == hipSuccess) e = o->grad.alloc(floats);
    if (e == hipSuccess) e = o->state.alloc(slots);
    if (e == hipSuccess) e = o->table.alloc(entries);
    if (e == hipSuccess) e = hipStreamSynchronize(dev->stream);
    if (e == hipSuccess) e = hipMemset(o->m, 0, floats * sizeof(float));
    if (e == hipSuccess) e = hipMemset(o->v, 0, floats * sizeof(float));
    if (e == hipSuccess && zero_grad) e = hipMemset(o->grad, 0, floats * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(o->state, st.data(), (size_t)slots * sizeof(rq::AdamState), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(o->table, table.data(), entries * sizeof(rq::PackGather), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? RQ_ERR_OUT_OF_MEMORY : RQ_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    return RQ_OK;
}

// k_adam_repack has written w_dev and both fp32 images (rq_trajectory_distill, rq_optimizer_apply): everything derived from the
// weights is behind - the host's mirror, the 16-bit images, a speculation or a saved state stamped with the old versions
void policy_updated_on_device(rq_policy* pol) {
    pol->version = fresh_version();
    pol->weight_version = fresh_version();
    pol->grad_image_version = pol->weight_version;
    pol->mirror_stale = pol->images16_stale = true;
}

// Adam's state of `slots` policies to the host, behind everything enqueued: m, v [slots][2084], step [slots], beta_powers [slots][2]
// (beta1^t, beta2^t as the kernel carries them).  Nothing of the caller's is written before every copy has arrived.
int adam_get_state(const char* who, AdamBuffers* o, uint32_t slots, float* m, float* v, uint32_t* step, double* beta_powers) {
    const size_t floats = (size_t)slots * RQ_POLICY_NUM_WEIGHTS;
    std::vector<rq::AdamState> st;
    std::vector<float> mv;
    try { st.resize(slots); mv.resize(2 * floats); } catch (const std::bad_alloc&) {
        return fail(RQ_ERR_OUT_OF_MEMORY, std::string(who) + ": host allocation failed");
    }
    hipStream_t s = o->dev->stream;
    RQ_HIP_AS(who, hipMemcpyAsync(mv.data(), o->m, floats * sizeof(float), hipMemcpyDeviceToHost, s));
    RQ_HIP_AS(who, hipMemcpyAsync(mv.data() + floats, o->v, floats * sizeof(float), hipMemcpyDeviceToHost, s));
    RQ_HIP_AS(who, hipMemcpyAsync(st.data(), o->state, (size_t)slots * sizeof(rq::AdamState), hipMemcpyDeviceToHost, s));
    RQ_HIP_AS(who, hipStreamSynchronize(s));
    std::memcpy(m, mv.data(), floats * sizeof(float));
    std::memcpy(v, mv.data() + floats, floats * sizeof(float));
    for (uint32_t p = 0; p < slots; ++p) {
        step[p] = st[p].step;
        beta_powers[2 * p] = st[p].beta1_t; beta_powers[2 * p + 1] = st[p].beta2_t;
    }
    return RQ_OK;
}

// The reverse, synchronous: the bits of m, v, step and the two powers as given; the hyper-parameters stay the optimizer's own
// (they are read back from the device first: a rq_*_set_lr enqueued before holds).
int adam_set_state(const char* who, AdamBuffers* o, uint32_t slots, const float* m, const float* v, const uint32_t* step,
                   const double* beta_powers) {
    const size_t floats = (size_t)slots * RQ_POLICY_NUM_WEIGHTS;
    std::vector<rq::AdamState> st;
    try { st.resize(slots); } catch (const std::bad_alloc&) {
        return fail(RQ_ERR_OUT_OF_MEMORY, std::string(who) + ": host allocation failed");
    }
    RQ_HIP_AS(who, hipStreamSynchronize(o->dev->stream));         // an update in flight reads and writes the state
    RQ_HIP_AS(who, hipMemcpy(st.data(), o->state, (size_t)slots * sizeof(rq::AdamState), hipMemcpyDeviceToHost));
    for (uint32_t p = 0; p < slots; ++p) {
        st[p].step = step[p];
        st[p].beta1_t = beta_powers[2 * p]; st[p].beta2_t = beta_powers[2 * p + 1];
    }
    RQ_HIP_AS(who, hipMemcpy(o->m, m, floats * sizeof(float), hipMemcpyHostToDevice));
    RQ_HIP_AS(who, hipMemcpy(o->v, v, floats * sizeof(float), hipMemcpyHostToDevice));
    RQ_HIP_AS(who, hipMemcpy(o->state, st.data(), (size_t)slots * sizeof(rq::AdamState), hipMemcpyHostToDevice));
    return RQ_OK;
}

// what the single optimizer's state calls and rq_optimizer_apply refuse alike: objects die in any order
int optimizer_check_policy(const rq_optimizer* opt, const char* what) {
    RQ_REFUSE(what, policy_registry(opt->policy, 0) && device_registry(opt->dev, 0), RQ_ERR_INVALID_ARGUMENT,
              "the optimizer's policy was destroyed");
    return RQ_OK;
}

int bank_optimizer_check_bank(const rq_bank_optimizer* opt, const char* what) {
    RQ_REFUSE(what, policy_bank_registry(opt->bank, 0) && opt->bank->uid == opt->bank_uid && device_registry(opt->dev, 0),
              RQ_ERR_INVALID_ARGUMENT, "the optimizer's bank was destroyed");
    return RQ_OK;
}

template <typename Optimizer>
int adam_destroy(Optimizer* opt) {
    if (!opt) return RQ_OK;
    DeviceScope on_device(opt->ordinal);
    if (device_registry(opt->dev, 0)) (void)hipStreamSynchronize(opt->dev->stream);      // an update may still be queued
    delete opt;
    return RQ_OK;
}

}  // namespace

extern "C" {

RQ_API int rq_trajectory_policy_forward(rq_trajectory* t, rq_policy* pol, int start, float* action, uint32_t ld_action,
                                        int memory) {
    int rc = grad_check_pair(t, pol, "rq_trajectory_policy_forward"); if (rc) return rc;
    rc = check_memory(memory); if (rc) return rc;
    RQ_REQUIRE(action, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(start == RQ_GRAD_START_CURRENT || start == RQ_GRAD_START_INITIAL, RQ_ERR_INVALID_ARGUMENT,
               "start must be RQ_GRAD_START_CURRENT or RQ_GRAD_START_INITIAL");
    rq_env* env = t->env;
    rq_device* dev = env->dev;
    RQ_REQUIRE(ld_action >= env->n, RQ_ERR_INVALID_ARGUMENT, "ld_action must be at least the number of envs");
    DeviceScope on_device(dev); rc = on_device.rc; if (rc) return rc;
    const uint32_t T = t->length, ld = env->ld;
    CallMemory mem(memory, dev->stream, dev->ordinal);
    if (start == RQ_GRAD_START_CURRENT) { rc = policy_size(pol, env->n); if (rc) return rc; }
    rc = ensure_grad_image(pol); if (rc) return rc;
    t->grad.valid = false;
    RQ_HIP(t->grad.saved.reserve(dev->stream, (size_t)T * RQ_POLICY_HIDDEN_DIM * ld));
    if (mem.host()) RQ_HIP(t->grad.rows.reserve(dev->stream, (size_t)T * RQ_ACTION_DIM * ld_action));
    // the envs' columns only go back: the caller's columns n .. ld_action-1 stay as they were
    float* d_act = mem.out(action, ld_action, t->grad.rows.get(), ld_action, env->n, (size_t)T * RQ_ACTION_DIM);
    RQ_HIP(rq::launch_policy_grad_forward(dev->stream, env->n, ld, T, pol->w_packed, t->obs, t->done,
                                          start == RQ_GRAD_START_CURRENT ? pol->hidden : nullptr, pol->ld,
                                          start == RQ_GRAD_START_INITIAL, d_act, ld_action, t->grad.saved));
    t->grad.stamp(pol, T, start);
    RQ_HIP(mem.finish());
    return RQ_OK;
}

RQ_API int rq_trajectory_policy_backward(rq_trajectory* t, rq_policy* pol, const float* grad_action, uint32_t ld_grad,
                                         float* grad_weights, float* grad_hidden_start, int memory) {
    int rc = grad_check_pair(t, pol, "rq_trajectory_policy_backward"); if (rc) return rc;
    rc = check_memory(memory); if (rc) return rc;
    RQ_REQUIRE(grad_action && grad_weights, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(t->grad.matches(pol, t->length), RQ_ERR_INVALID_ARGUMENT,
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
    CallMemory mem(memory, dev->stream, dev->ordinal);
    RQ_HIP(t->grad.partial.reserve(dev->stream, (size_t)waves * RQ_POLICY_NUM_WEIGHTS));
    const size_t ga_floats = (size_t)T * RQ_ACTION_DIM * ld_grad, gh_floats = (size_t)RQ_POLICY_HIDDEN_DIM * ld;
    float *s_ga = nullptr, *s_gw = nullptr, *s_gh = nullptr;
    if (mem.host()) {          // one device block: dL/da | dL/dtheta | dL/dh_start, each begun at a multiple of 256 bytes
        const size_t off_gw = (ga_floats + 63) & ~(size_t)63, off_gh = off_gw + ((RQ_POLICY_NUM_WEIGHTS + 63) & ~(size_t)63);
        RQ_HIP(t->grad.rows.reserve(dev->stream, off_gh + gh_floats));
        s_ga = t->grad.rows; s_gw = s_ga + off_gw; s_gh = s_ga + off_gh;
    }
    const float* d_ga = nullptr; RQ_HIP(mem.in(grad_action, ga_floats, s_ga, &d_ga));
    float* d_gw = mem.out(grad_weights, RQ_POLICY_NUM_WEIGHTS, s_gw);
    float* d_gh = grad_hidden_start ? mem.out(grad_hidden_start, gh_floats, s_gh) : nullptr;
    RQ_HIP(rq::launch_policy_grad_backward(dev->stream, env->n, ld, T, pol->w_packed, pol->w_packed_grad, t->obs, t->done,
                                           t->grad.saved, d_ga, ld_grad, t->grad.start == RQ_GRAD_START_INITIAL, d_gh,
                                           t->grad.partial, d_gw));
    RQ_HIP(mem.finish());
    return RQ_OK;
}

// ---------------------------------------------------------------------------- the update on the device ---
// Each call and its *_weighted sibling are one body: `wt` is kNoWeight or the sibling's weight, `what` the name in the messages.
static int policy_loss_grad(rq_trajectory* t, rq_policy* pol, const float* target, uint32_t ld_target, const LossWeight& wt, int start,
                            float* loss, float* grad_weights, int memory, const char* what) {
    RQ_REQUIRE(t && pol && loss && grad_weights, RQ_ERR_INVALID_ARGUMENT, "null argument");
    int rc = loss_check(t, pol, target, ld_target, wt, start, memory, what); if (rc) return rc;
    rq_device* dev = t->env->dev;
    DeviceScope on_device(dev); rc = on_device.rc; if (rc) return rc;
    CallMemory mem(memory, dev->stream, dev->ordinal);
    rq::LossLaunch a;
    rc = loss_begin(t, pol, target, ld_target, wt, start, mem, 1, &a); if (rc) return rc;
    a.grad = mem.out(grad_weights, RQ_POLICY_NUM_WEIGHTS, t->grad.out.get());
    a.loss = mem.out(loss, 1, t->grad.out.get() + RQ_POLICY_NUM_WEIGHTS);
    RQ_HIP(rq::launch_policy_loss_grad(dev->stream, a));
    t->grad.stamp(pol, t->length, start);          // the saved state is the forward's: a rq_trajectory_policy_backward may follow
    RQ_HIP(mem.finish());
    return RQ_OK;
}

RQ_API int rq_trajectory_policy_loss_grad(rq_trajectory* t, rq_policy* pol, const float* target, uint32_t ld_target, int start,
                                          float* loss, float* grad_weights, int memory) {
    return policy_loss_grad(t, pol, target, ld_target, kNoWeight, start, loss, grad_weights, memory, "rq_trajectory_policy_loss_grad");
}

RQ_API int rq_trajectory_policy_loss_grad_weighted(rq_trajectory* t, rq_policy* pol, const float* target, uint32_t ld_target,
                                                   const float* weight, uint32_t ld_weight, uint32_t weight_steps, int start,
                                                   float* loss, float* grad_weights, int memory) {
    return policy_loss_grad(t, pol, target, ld_target, LossWeight{true, weight, ld_weight, weight_steps}, start, loss, grad_weights,
                            memory, "rq_trajectory_policy_loss_grad_weighted");
}

RQ_API int rq_optimizer_create(rq_policy* pol, const rq_adam_config* config, rq_optimizer** out) {
    RQ_REQUIRE(pol && config && out, RQ_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    RQ_REQUIRE(adam_config_ok(*config), RQ_ERR_INVALID_ARGUMENT, "lr, eps and weight_decay must be non-negative and the betas in [0, 1)");
    rq_device* dev = pol->dev;
    DeviceScope on_device(dev); int rc = on_device.rc; if (rc) return rc;
    rq_optimizer* o = new (std::nothrow) rq_optimizer();
    RQ_REQUIRE(o, RQ_ERR_OUT_OF_MEMORY, "host allocation failed");
    o->policy = pol;
    rc = adam_alloc("rq_optimizer_create", o, dev, config, 1, 1, false);
    if (rc) { delete o; return rc; }
    *out = o;
    return RQ_OK;
}

RQ_API int rq_optimizer_destroy(rq_optimizer* opt) { return adam_destroy(opt); }

RQ_API int rq_optimizer_set_lr(rq_optimizer* opt, double lr) {
    RQ_REQUIRE(opt, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(lr >= 0.0, RQ_ERR_INVALID_ARGUMENT, "lr must be non-negative");
    DeviceScope on_device(opt->dev); int rc = on_device.rc; if (rc) return rc;
    RQ_HIP(rq::launch_adam_set_lr(opt->dev->stream, opt->state, lr));
    return RQ_OK;
}

RQ_API int rq_optimizer_get_state(rq_optimizer* opt, float* m, float* v, uint32_t* step, double* beta_powers) {
    RQ_REQUIRE(opt && m && v && step && beta_powers, RQ_ERR_INVALID_ARGUMENT, "null argument");
    int rc = optimizer_check_policy(opt, "rq_optimizer_get_state"); if (rc) return rc;
    DeviceScope on_device(opt->ordinal); rc = on_device.rc; if (rc) return rc;
    return adam_get_state("rq_optimizer_get_state", opt, 1, m, v, step, beta_powers);
}

RQ_API int rq_optimizer_set_state(rq_optimizer* opt, const float* m, const float* v, uint32_t step, const double* beta_powers) {
    RQ_REQUIRE(opt && m && v && beta_powers, RQ_ERR_INVALID_ARGUMENT, "null argument");
    int rc = optimizer_check_policy(opt, "rq_optimizer_set_state"); if (rc) return rc;
    DeviceScope on_device(opt->ordinal); rc = on_device.rc; if (rc) return rc;
    return adam_set_state("rq_optimizer_set_state", opt, 1, m, v, &step, beta_powers);
}

RQ_API int rq_optimizer_apply(rq_optimizer* opt, const float* grad, int memory) {
    const char* what = "rq_optimizer_apply";
    RQ_REQUIRE(opt && grad, RQ_ERR_INVALID_ARGUMENT, "null argument");
    int rc = check_memory(memory); if (rc) return rc;
    rc = optimizer_check_policy(opt, what); if (rc) return rc;
    rq_policy* pol = opt->policy;
    rq_device* dev = opt->dev;
    // the kernel rebuilds the fp32 images from the raw weights: as rq_trajectory_distill, the fp32 policy without a folded stage only
    RQ_REQUIRE(pol->precision == RQ_POLICY_FP32, RQ_ERR_INVALID_ARGUMENT,
               std::string(what) + ": defined for the fp32 policy only (set_precision(RQ_POLICY_FP32)), not bf16 or f16x2");
    RQ_REQUIRE(!pol->standardize, RQ_ERR_INVALID_ARGUMENT, std::string(what) + ": the Standardize stage has no gradient here (disable it)");
    CallMemory mem(memory, dev->stream, dev->ordinal);
    rc = check_device_array(mem, grad, what, "the gradient"); if (rc) return rc;
    rc = check_host_array(mem, grad, what, "the gradient"); if (rc) return rc;
    DeviceScope on_device(dev); rc = on_device.rc; if (rc) return rc;          // (retires a resident executor: it holds the old operands)
    rc = ensure_grad_image(pol); if (rc) return rc;                            // the kernel writes both images: the second must exist
    const float* d_grad = nullptr;
    RQ_HIP(mem.in(grad, (size_t)RQ_POLICY_NUM_WEIGHTS, opt->grad.get(), &d_grad));
    const hipError_t e = rq::launch_adam_repack(dev->stream, d_grad, pol->w_dev, opt->m, opt->v, opt->state, opt->table, pol->w_packed,
                                                pol->w_packed_grad);
    if (e == hipSuccess) policy_updated_on_device(pol);
    RQ_HIP(e);
    RQ_HIP(mem.finish());
    return RQ_OK;
}

static int policy_distill(rq_trajectory* t, rq_policy* pol, rq_optimizer* opt, const float* target, uint32_t ld_target,
                          const LossWeight& wt, int start, uint32_t n_updates, float* losses, int memory, const char* what) {
    RQ_REQUIRE(t && pol && opt && losses, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(policy_registry(pol, 0) && opt->policy == pol, RQ_ERR_INVALID_ARGUMENT,
               std::string(what) + ": the optimizer was made for another policy");
    RQ_REQUIRE(n_updates > 0, RQ_ERR_INVALID_ARGUMENT, "n_updates must be positive");
    int rc = loss_check(t, pol, target, ld_target, wt, start, memory, what); if (rc) return rc;
    rq_device* dev = t->env->dev;
    DeviceScope on_device(dev); rc = on_device.rc; if (rc) return rc;          // (retires a resident executor: it holds the old operands)
    CallMemory mem(memory, dev->stream, dev->ordinal);
    rq::LossLaunch a;
    rc = loss_begin(t, pol, target, ld_target, wt, start, mem, n_updates, &a); if (rc) return rc;
    a.grad = opt->grad;
    float* d_losses = mem.out(losses, n_updates, t->grad.out.get() + RQ_POLICY_NUM_WEIGHTS);
    hipError_t e = hipSuccess;
    uint32_t done_updates = 0;
    for (; done_updates < n_updates && e == hipSuccess; ++done_updates) {
        a.loss = d_losses + done_updates;
        e = rq::launch_policy_loss_grad(dev->stream, a);
        if (e == hipSuccess) e = rq::launch_adam_repack(dev->stream, opt->grad, pol->w_dev, opt->m, opt->v, opt->state, opt->table,
                                                        pol->w_packed, pol->w_packed_grad);
    }
    if (done_updates > 0) policy_updated_on_device(pol);      // (even if a later launch failed)
    RQ_HIP(e);
    RQ_HIP(mem.finish());
    return RQ_OK;
}

RQ_API int rq_trajectory_distill(rq_trajectory* t, rq_policy* pol, rq_optimizer* opt, const float* target, uint32_t ld_target,
                                 int start, uint32_t n_updates, float* losses, int memory) {
    return policy_distill(t, pol, opt, target, ld_target, kNoWeight, start, n_updates, losses, memory, "rq_trajectory_distill");
}

RQ_API int rq_trajectory_distill_weighted(rq_trajectory* t, rq_policy* pol, rq_optimizer* opt, const float* target, uint32_t ld_target,
                                          const float* weight, uint32_t ld_weight, uint32_t weight_steps, int start,
                                          uint32_t n_updates, float* losses, int memory) {
    return policy_distill(t, pol, opt, target, ld_target, LossWeight{true, weight, ld_weight, weight_steps}, start, n_updates, losses,
                          memory, "rq_trajectory_distill_weighted");
}

// ---------------------------------------------------------------------------- the update on the device, a bank at once ---
static int policies_loss_grad(rq_trajectory* t, rq_policy_bank* bank, const uint32_t* policy_id, const float* target,
                              uint32_t ld_target, const LossWeight& wt, int start, float* loss, float* grad_weights, int memory,
                              const char* what) {
    RQ_REQUIRE(t && bank && policy_id && loss && grad_weights, RQ_ERR_INVALID_ARGUMENT, "null argument");
    int rc = bank_loss_check(t, bank, policy_id, target, ld_target, wt, start, memory, what); if (rc) return rc;
    rq_device* dev = t->env->dev;
    DeviceScope on_device(dev); rc = on_device.rc; if (rc) return rc;
    const size_t P = bank->n_policies, grad_floats = P * RQ_POLICY_NUM_WEIGHTS;
    CallMemory mem(memory, dev->stream, dev->ordinal);
    rq::LossLaunch a;
    rc = bank_loss_begin(t, bank, policy_id, target, ld_target, wt, start, mem, P, &a); if (rc) return rc;
    float* d_grad = a.grad = mem.host() ? t->grad.out.get() : grad_weights;
    a.loss = mem.out(loss, P, t->grad.out.get() + grad_floats);
    RQ_HIP(rq::launch_policy_loss_grad(dev->stream, a));
    // (t->grad.valid stays false: the saved state is no single policy's, rq_trajectory_policy_backward has nothing to follow)
    if (mem.host()) {
        // a policy that owns no wave has no gradient row on the device: the caller's row stays as it was (the losses: finish)
        std::vector<uint32_t> owns;
        try { owns.assign(P, 0u); } catch (const std::bad_alloc&) { return fail(RQ_ERR_OUT_OF_MEMORY, "host allocation failed"); }
        for (uint32_t id : bank->table_ids) owns[id] = 1u;
        for (size_t p = 0; p < P; ++p)
            if (owns[p])
                RQ_HIP(hipMemcpyAsync(grad_weights + p * RQ_POLICY_NUM_WEIGHTS, d_grad + p * RQ_POLICY_NUM_WEIGHTS,
                                      RQ_POLICY_NUM_WEIGHTS * sizeof(float), hipMemcpyDeviceToHost, dev->stream));
    }
    RQ_HIP(mem.finish());
    return RQ_OK;
}

RQ_API int rq_trajectory_policies_loss_grad(rq_trajectory* t, rq_policy_bank* bank, const uint32_t* policy_id, const float* target,
                                            uint32_t ld_target, int start, float* loss, float* grad_weights, int memory) {
    return policies_loss_grad(t, bank, policy_id, target, ld_target, kNoWeight, start, loss, grad_weights, memory,
                              "rq_trajectory_policies_loss_grad");
}

RQ_API int rq_trajectory_policies_loss_grad_weighted(rq_trajectory* t, rq_policy_bank* bank, const uint32_t* policy_id,
                                                     const float* target, uint32_t ld_target, const float* weight, uint32_t ld_weight,
                                                     uint32_t weight_steps, int start, float* loss, float* grad_weights, int memory) {
    return policies_loss_grad(t, bank, policy_id, target, ld_target, LossWeight{true, weight, ld_weight, weight_steps}, start, loss,
                              grad_weights, memory, "rq_trajectory_policies_loss_grad_weighted");
}

RQ_API int rq_bank_optimizer_create(rq_policy_bank* bank, const rq_adam_config* config, uint32_t n_cfg, rq_bank_optimizer** out) {
    RQ_REQUIRE(bank && config && out, RQ_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    const uint32_t P = bank->n_policies;
    RQ_REQUIRE(n_cfg == 1 || n_cfg == P, RQ_ERR_INVALID_ARGUMENT,
               "n_cfg must be 1 (one configuration for every policy) or the bank's " + std::to_string(P) + " policies, not " + std::to_string(n_cfg));
    for (uint32_t k = 0; k < n_cfg; ++k)
        RQ_REQUIRE(adam_config_ok(config[k]), RQ_ERR_INVALID_ARGUMENT,
                   "lr, eps and weight_decay must be non-negative and the betas in [0, 1) (configuration " + std::to_string(k) + ")");
    rq_device* dev = bank->dev;
    DeviceScope on_device(dev); int rc = on_device.rc; if (rc) return rc;
    rq_bank_optimizer* o = new (std::nothrow) rq_bank_optimizer();
    RQ_REQUIRE(o, RQ_ERR_OUT_OF_MEMORY, "host allocation failed");
    o->bank = bank; o->bank_uid = bank->uid; o->n_policies = P;
    rc = adam_alloc("rq_bank_optimizer_create", o, dev, config, n_cfg, P, true);
    if (rc) { delete o; return rc; }
    *out = o;
    return RQ_OK;
}

RQ_API int rq_bank_optimizer_destroy(rq_bank_optimizer* opt) { return adam_destroy(opt); }

RQ_API int rq_bank_optimizer_set_lr(rq_bank_optimizer* opt, const double* lr, uint32_t n) {
    RQ_REQUIRE(opt && lr, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(n == 1 || n == opt->n_policies, RQ_ERR_INVALID_ARGUMENT,
               "n must be 1 (one rate for every policy) or the bank's " + std::to_string(opt->n_policies) + " policies, not " + std::to_string(n));
    for (uint32_t k = 0; k < n; ++k) RQ_REQUIRE(lr[k] >= 0.0, RQ_ERR_INVALID_ARGUMENT, "lr must be non-negative");
    DeviceScope on_device(opt->dev); int rc = on_device.rc; if (rc) return rc;
    RQ_HIP(rq::launch_adam_set_lr_bank(opt->dev->stream, opt->state, opt->n_policies, lr, n));
    return RQ_OK;
}

RQ_API int rq_bank_optimizer_get_state(rq_bank_optimizer* opt, float* m, float* v, uint32_t* step, double* beta_powers) {
    RQ_REQUIRE(opt && m && v && step && beta_powers, RQ_ERR_INVALID_ARGUMENT, "null argument");
    int rc = bank_optimizer_check_bank(opt, "rq_bank_optimizer_get_state"); if (rc) return rc;
    DeviceScope on_device(opt->ordinal); rc = on_device.rc; if (rc) return rc;
    return adam_get_state("rq_bank_optimizer_get_state", opt, opt->n_policies, m, v, step, beta_powers);
}

RQ_API int rq_bank_optimizer_set_state(rq_bank_optimizer* opt, const float* m, const float* v, const uint32_t* step,
                                       const double* beta_powers) {
    RQ_REQUIRE(opt && m && v && step && beta_powers, RQ_ERR_INVALID_ARGUMENT, "null argument");
    int rc = bank_optimizer_check_bank(opt, "rq_bank_optimizer_set_state"); if (rc) return rc;
    DeviceScope on_device(opt->ordinal); rc = on_device.rc; if (rc) return rc;
    return adam_set_state("rq_bank_optimizer_set_state", opt, opt->n_policies, m, v, step, beta_powers);
}

static int policies_distill(rq_trajectory* t, rq_policy_bank* bank, rq_bank_optimizer* opt, const uint32_t* policy_id,
                            const float* target, uint32_t ld_target, const LossWeight& wt, int start, uint32_t n_updates,
                            float* losses, int memory, const char* what) {
    RQ_REQUIRE(t && bank && opt && policy_id && losses, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(opt->bank == bank && opt->bank_uid == bank->uid, RQ_ERR_INVALID_ARGUMENT,
               std::string(what) + ": the optimizer was made for another bank");
    RQ_REQUIRE(n_updates > 0, RQ_ERR_INVALID_ARGUMENT, "n_updates must be positive");
    int rc = bank_loss_check(t, bank, policy_id, target, ld_target, wt, start, memory, what); if (rc) return rc;
    rq_device* dev = t->env->dev;
    DeviceScope on_device(dev); rc = on_device.rc; if (rc) return rc;
    const size_t P = bank->n_policies, n_losses = (size_t)n_updates * P;
    CallMemory mem(memory, dev->stream, dev->ordinal);
    rq::LossLaunch a;
    rc = bank_loss_begin(t, bank, policy_id, target, ld_target, wt, start, mem, n_losses, &a); if (rc) return rc;
    a.grad = opt->grad;
    float* d_losses = mem.out(losses, n_losses, t->grad.out.get() + P * RQ_POLICY_NUM_WEIGHTS);
    hipError_t e = hipSuccess;
    for (uint32_t k = 0; k < n_updates && e == hipSuccess; ++k) {       // back to back: nothing waits in between
        a.loss = d_losses + (size_t)k * P;
        e = rq::launch_policy_loss_grad(dev->stream, a);
        if (e == hipSuccess) e = rq::launch_adam_repack_bank(dev->stream, bank->n_policies, bank->waves, opt->grad, bank->weights, opt->m,
                                                             opt->v, opt->state, opt->table, bank->images, bank->gimages);
    }
    RQ_HIP(e);
    RQ_HIP(mem.finish());
    return RQ_OK;
}

RQ_API int rq_trajectory_policies_distill(rq_trajectory* t, rq_policy_bank* bank, rq_bank_optimizer* opt, const uint32_t* policy_id,
                                          const float* target, uint32_t ld_target, int start, uint32_t n_updates, float* losses,
                                          int memory) {
    return policies_distill(t, bank, opt, policy_id, target, ld_target, kNoWeight, start, n_updates, losses, memory,
                            "rq_trajectory_policies_distill");
}

RQ_API int rq_trajectory_policies_distill_weighted(rq_trajectory* t, rq_policy_bank* bank, rq_bank_optimizer* opt,
                                                   const uint32_t* policy_id, const float* target, uint32_t ld_target,
                                                   const float* weight, uint32_t ld_weight, uint32_t weight_steps, int start,
                                                   uint32_t n_updates, float* losses, int memory) {
    return policies_distill(t, bank, opt, policy_id, target, ld_target, LossWeight{true, weight, ld_weight, weight_steps}, start,
                            n_updates, losses, memory, "rq_trajectory_policies_distill_weighted");
}

// ---------------------------------------------------------------------------- the imitation error table ---
RQ_API int rq_trajectory_policy_error_table(rq_trajectory* t, rq_policy* pol, const float* target, uint32_t ld_target,
                                            const uint32_t* age_edges, uint32_t n_buckets, int start, float* sse, uint32_t* count,
                                            uint32_t ld_out, int memory) {
    const char* what = __func__;
    RQ_REQUIRE(t && pol, RQ_ERR_INVALID_ARGUMENT, "null argument");
    int rc = loss_check(t, pol, target, ld_target, kNoWeight, start, memory, what); if (rc) return rc;
    rq::ErrorTableLaunch a;
    rc = error_table_check(what, t, target, age_edges, n_buckets, sse, count, ld_out, memory, &a); if (rc) return rc;
    rq_device* dev = t->env->dev;
    DeviceScope on_device(dev); rc = on_device.rc; if (rc) return rc;
    CallMemory mem(memory, dev->stream, dev->ordinal);
    if (start == RQ_GRAD_START_CURRENT) { rc = policy_size(pol, t->env->n); if (rc) return rc; }
    rc = error_table_begin(t, target, ld_target, start, mem, sse, count, ld_out, &a); if (rc) return rc;
    a.pass.packed = pol->w_packed;
    a.pass.hidden = start == RQ_GRAD_START_CURRENT ? pol->hidden.get() : nullptr;
    a.pass.ld_h = pol->ld;
    RQ_HIP(rq::launch_policy_error_table(dev->stream, a));
    RQ_HIP(mem.finish());
    return RQ_OK;
}

RQ_API int rq_trajectory_policies_error_table(rq_trajectory* t, rq_policy_bank* bank, const uint32_t* policy_id, const float* target,
                                              uint32_t ld_target, const uint32_t* age_edges, uint32_t n_buckets, int start, float* sse,
                                              uint32_t* count, uint32_t ld_out, int memory) {
    const char* what = __func__;
    RQ_REQUIRE(t && bank && policy_id, RQ_ERR_INVALID_ARGUMENT, "null argument");
    int rc = bank_loss_check(t, bank, policy_id, target, ld_target, kNoWeight, start, memory, what); if (rc) return rc;
    rq::ErrorTableLaunch a;
    rc = error_table_check(what, t, target, age_edges, n_buckets, sse, count, ld_out, memory, &a); if (rc) return rc;
    rq_env* env = t->env;
    rq_device* dev = env->dev;
    DeviceScope on_device(dev); rc = on_device.rc; if (rc) return rc;
    CallMemory mem(memory, dev->stream, dev->ordinal);
    if (start == RQ_GRAD_START_CURRENT) {
        rc = bank_size(bank, env->n); if (rc) return rc;
        RQ_REQUIRE(bank->ld == env->ld, RQ_ERR_SHAPE_MISMATCH, "policy bank batch does not match the env");
    }
    rc = bank_table(bank, dev, env->uid, policy_id, env->n); if (rc) return rc;
    if (start == RQ_GRAD_START_CURRENT) { rc = bank_apply_reset(bank); if (rc) return rc; }
    rc = error_table_begin(t, target, ld_target, start, mem, sse, count, ld_out, &a); if (rc) return rc;
    a.pass.packed = bank->images;
    a.pass.n_policies = bank->n_policies; a.pass.block_policy = bank->table;
    a.pass.hidden = start == RQ_GRAD_START_CURRENT ? bank->hidden.get() : nullptr;
    a.pass.ld_h = bank->ld;
    RQ_HIP(rq::launch_policy_error_table(dev->stream, a));
    RQ_HIP(mem.finish());
    return RQ_OK;
}

// ---------------------------------------------------------------------------- the feedback-gain table ---
RQ_API int rq_trajectory_policy_gain_table(rq_trajectory* t, rq_policy* pol, const uint32_t* age_edges, uint32_t n_buckets, int start,
                                           float* sum, uint32_t* count, uint32_t ld_out, int memory) {
    const char* what = __func__;
    RQ_REQUIRE(t && pol, RQ_ERR_INVALID_ARGUMENT, "null argument");
    int rc = loss_check(t, pol, nullptr, 0, kNoWeight, start, memory, what); if (rc) return rc;
    rq::GainTableLaunch a;
    rc = error_table_check(what, t, nullptr, age_edges, n_buckets, sum, count, ld_out, memory, &a, "sum"); if (rc) return rc;
    rq_device* dev = t->env->dev;
    DeviceScope on_device(dev); rc = on_device.rc; if (rc) return rc;
    CallMemory mem(memory, dev->stream, dev->ordinal);
    if (start == RQ_GRAD_START_CURRENT) { rc = policy_size(pol, t->env->n); if (rc) return rc; }
    rc = ensure_grad_image(pol); if (rc) return rc;
    rc = gain_table_begin(t, start, mem, sum, count, ld_out, &a); if (rc) return rc;
    a.pass.packed = pol->w_packed; a.pass.gpacked = pol->w_packed_grad;
    a.pass.hidden = start == RQ_GRAD_START_CURRENT ? pol->hidden.get() : nullptr;
    a.pass.ld_h = pol->ld;
    RQ_HIP(rq::launch_policy_gain_table(dev->stream, a));
    RQ_HIP(mem.finish());
    return RQ_OK;
}

RQ_API int rq_trajectory_policies_gain_table(rq_trajectory* t, rq_policy_bank* bank, const uint32_t* policy_id, const uint32_t* age_edges,
                                             uint32_t n_buckets, int start, float* sum, uint32_t* count, uint32_t ld_out, int memory) {
    const char* what = __func__;
    RQ_REQUIRE(t && bank && policy_id, RQ_ERR_INVALID_ARGUMENT, "null argument");
    int rc = bank_loss_check(t, bank, policy_id, nullptr, 0, kNoWeight, start, memory, what); if (rc) return rc;
    rq::GainTableLaunch a;
    rc = error_table_check(what, t, nullptr, age_edges, n_buckets, sum, count, ld_out, memory, &a, "sum"); if (rc) return rc;
    rq_env* env = t->env;
    rq_device* dev = env->dev;
    DeviceScope on_device(dev); rc = on_device.rc; if (rc) return rc;
    CallMemory mem(memory, dev->stream, dev->ordinal);
    if (start == RQ_GRAD_START_CURRENT) {
        rc = bank_size(bank, env->n); if (rc) return rc;
        RQ_REQUIRE(bank->ld == env->ld, RQ_ERR_SHAPE_MISMATCH, "policy bank batch does not match the env");
    }
    rc = bank_table(bank, dev, env->uid, policy_id, env->n); if (rc) return rc;
    rc = bank_grad_images(bank); if (rc) return rc;
    if (start == RQ_GRAD_START_CURRENT) { rc = bank_apply_reset(bank); if (rc) return rc; }
    rc = gain_table_begin(t, start, mem, sum, count, ld_out, &a); if (rc) return rc;
    a.pass.packed = bank->images; a.pass.gpacked = bank->gimages;
    a.pass.n_policies = bank->n_policies; a.pass.block_policy = bank->table;
    a.pass.hidden = start == RQ_GRAD_START_CURRENT ? bank->hidden.get() : nullptr;
    a.pass.ld_h = bank->ld;
    RQ_HIP(rq::launch_policy_gain_table(dev->stream, a));
    RQ_HIP(mem.finish());
    return RQ_OK;
}

}  // extern "C"
