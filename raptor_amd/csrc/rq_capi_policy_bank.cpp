// rq_capi_policy_bank.cpp - the policy bank: P fp32 student policies (checkpoints of a run, a sweep, a seed population) flown in ONE
// rollout, one policy per 64-env block (= per wave of the fused kernel).  The student-side mirror of the teacher bank's rollout
// (rq_capi_teacher.cpp): same frame (rollout_run), the id table cached in the bank.
#include "rq_objects.hpp"

using namespace rqh;

namespace {

constexpr const char* kWeightsShape = "expected 2084 weights per policy: W0[16,22] b0[16] Wi[48,16] Wh[48,16] bi[48] bh[48] h0[16] W2[4,16] b2[4]";

inline uint32_t blocks_of(uint32_t n) { return (n + 63u) / 64u; }

}  // namespace

namespace rqh {

// policy_id[0 .. n): every id names a policy of the bank and is constant on every aligned block of 64 (checked before anything is
// enqueued); the ragged last block is one block
int bank_check_ids(const rq_policy_bank* bank, const uint32_t* policy_id, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) {
        RQ_REQUIRE(policy_id[i] < bank->n_policies, RQ_ERR_INVALID_ARGUMENT,
                   "policy id out of range: env " + std::to_string(i) + " names policy " + std::to_string(policy_id[i]) + " of a bank of " +
                       std::to_string(bank->n_policies));
        RQ_REQUIRE(policy_id[i] == policy_id[i & ~63u], RQ_ERR_INVALID_ARGUMENT,
                   "policy ids differ inside a 64-env block: env " + std::to_string(i) + " names policy " + std::to_string(policy_id[i]) +
                       ", env " + std::to_string(i & ~63u) + " policy " + std::to_string(policy_id[i & ~63u]) +
                       " (a policy flies whole blocks of 64 envs: one wave, one operand image)");
    }
    return RQ_OK;
}

// The bank's device table of one id per block for the n envs assigned by policy_id, uploaded only when (key, ids) differ from what
// `table` holds.  Needs the caller's DeviceScope.
int bank_table(rq_policy_bank* bank, rq_device* dev, uint64_t key, const uint32_t* policy_id, uint32_t n) {
    const uint32_t blocks = blocks_of(n);
    bool same = bank->table_valid && bank->table_key == key && bank->table_ids.size() == blocks;
    for (uint32_t g = 0; same && g < blocks; ++g) same = bank->table_ids[g] == policy_id[(size_t)g * 64];
    if (same) return RQ_OK;
    bank->table_valid = bank->waves_valid = false;
    try {                                   // nothing throws across the boundary
        bank->table_ids.resize(blocks);
    } catch (const std::bad_alloc&) {
        return fail(RQ_ERR_OUT_OF_MEMORY, "policy bank: host allocation failed");
    }
    for (uint32_t g = 0; g < blocks; ++g) bank->table_ids[g] = policy_id[(size_t)g * 64];
    RQ_HIP(bank->table.reserve(dev->stream, blocks));
    RQ_HIP(hipMemcpyAsync(bank->table, bank->table_ids.data(), (size_t)blocks * sizeof(uint32_t), hipMemcpyHostToDevice, dev->stream));
    RQ_HIP(hipStreamSynchronize(dev->stream));                // table_ids is pageable, and may change before the copy would run
    bank->table_valid = true;
    bank->table_key = key;
    return RQ_OK;
}

// The hidden state sized on first use, as a policy's is (policy_size).  Needs the caller's DeviceScope.
int bank_size(rq_policy_bank* bank, uint32_t batch) {
    if (bank->batch == batch && bank->hidden) return RQ_OK;
    RQ_REQUIRE(bank->batch == 0 || bank->needs_reset, RQ_ERR_SHAPE_MISMATCH,
               "batch size changed without reset (hidden state is per batch element)");
    RQ_HIP(hipStreamSynchronize(bank->dev->stream));
    bank->hidden.reset();
    bank->batch = bank->ld = 0;                    // not sized, should the allocation fail
    const uint32_t ld = round_up64(batch);
    RQ_HIP(bank->hidden.alloc((size_t)RQ_POLICY_HIDDEN_DIM * ld));
    bank->batch = batch; bank->ld = ld;
    bank->needs_reset = true;
    return RQ_OK;
}

// a pending reset applied: every env's hidden state <- the initial state of the policy the table gives its block
int bank_apply_reset(rq_policy_bank* bank) {
    if (!bank->needs_reset) return RQ_OK;
    RQ_HIP(rq::launch_bank_initial_hidden(bank->dev->stream, bank->ld, bank->hidden, bank->weights, bank->table));
    bank->needs_reset = false;
    return RQ_OK;
}

// The learner's transposed images [P][RQ_PACKED_GRAD_FLOATS], packed once from the master weights ON THE DEVICE (set_weights and
// device-side updates have written there); from then on every writer of a slot's weights writes its transposed image too.
int bank_grad_images(rq_policy_bank* bank) {
    if (bank->gimages) return RQ_OK;
    const size_t P = bank->n_policies;
    std::vector<float> w, images;
    try { w.resize(P * RQ_POLICY_NUM_WEIGHTS); images.resize(P * rq::RQ_PACKED_GRAD_FLOATS); } catch (const std::bad_alloc&) {
        return fail(RQ_ERR_OUT_OF_MEMORY, "policy bank: host allocation failed");
    }
    RQ_HIP(hipStreamSynchronize(bank->dev->stream));
    RQ_HIP(hipMemcpy(w.data(), bank->weights, w.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < P; ++k) rq::pack_policy_grad(w.data() + k * RQ_POLICY_NUM_WEIGHTS, images.data() + k * rq::RQ_PACKED_GRAD_FLOATS);
    DeviceBuffer<float> d;
    RQ_HIP(d.alloc(images.size()));
    RQ_HIP(hipMemcpy(d, images.data(), images.size() * sizeof(float), hipMemcpyHostToDevice));
    bank->gimages = std::move(d);
    return RQ_OK;
}

// The policies' waves as a CSR list, from the table in place (bank_table first): wave_offsets [P + 1] | wave_list [blocks], the
// waves of a policy in ascending order.  Cached like the table: rebuilt only when bank_table uploaded another one.
int bank_wave_lists(rq_policy_bank* bank) {
    RQ_REQUIRE(bank->table_valid, RQ_ERR_NOT_INITIALIZED, "policy bank: no id table");
    if (bank->waves_valid) return RQ_OK;
    const uint32_t P = bank->n_policies, blocks = (uint32_t)bank->table_ids.size();
    std::vector<uint32_t> csr;
    try { csr.assign((size_t)P + 1 + blocks, 0u); } catch (const std::bad_alloc&) {
        return fail(RQ_ERR_OUT_OF_MEMORY, "policy bank: host allocation failed");
    }
    for (uint32_t g = 0; g < blocks; ++g) ++csr[bank->table_ids[g] + 1];              // counts, one slot up
    for (uint32_t p = 0; p < P; ++p) csr[p + 1] += csr[p];                            // -> offsets
    std::vector<uint32_t> fill(csr.begin(), csr.begin() + P);
    for (uint32_t g = 0; g < blocks; ++g) csr[(size_t)P + 1 + fill[bank->table_ids[g]]++] = g;     // block order: ascending per policy
    RQ_HIP(bank->waves.reserve(bank->dev->stream, csr.size()));
    RQ_HIP(hipMemcpyAsync(bank->waves, csr.data(), csr.size() * sizeof(uint32_t), hipMemcpyHostToDevice, bank->dev->stream));
    RQ_HIP(hipStreamSynchronize(bank->dev->stream));          // csr is pageable and goes away
    bank->waves_valid = true;
    return RQ_OK;
}

int require_bank_native_rate(const rq_policy_bank* bank, const char* what) {
    if (!bank->rated) return RQ_OK;
    uint32_t p = 0;
    while (p + 1 < bank->n_policies && bank->intervals[p] == 1) ++p;
    return fail(RQ_ERR_INVALID_ARGUMENT,
                std::string(what) + ": defined at the native rate only, policy " + std::to_string(p) + " of the bank has native interval " +
                    std::to_string(bank->intervals[p]) + " (rq_policy_bank_set_native_interval(bank, &one, 1) with one = 1)");
}

}  // namespace rqh

namespace {

// slot `index` of the device arrays from 2084 host weights (synchronous: the caller's array is its own again on return)
int bank_upload_slot(rq_policy_bank* bank, uint32_t index, const float* weights) {
    std::vector<float> image;
    try { image.resize(std::max<size_t>(rq::RQ_PACKED_FLOATS, rq::RQ_PACKED_GRAD_FLOATS)); } catch (const std::bad_alloc&) {
        return fail(RQ_ERR_OUT_OF_MEMORY, "policy bank: host allocation failed");
    }
    if (bank->gimages) {               // the learner has been used: its transposed image of the slot follows
        rq::pack_policy_grad(weights, image.data());
        RQ_HIP(hipMemcpy(bank->gimages + (size_t)index * rq::RQ_PACKED_GRAD_FLOATS, image.data(),
                         (size_t)rq::RQ_PACKED_GRAD_FLOATS * sizeof(float), hipMemcpyHostToDevice));
    }
    rq::pack_policy(weights, image.data());
    RQ_HIP(hipMemcpy(bank->images + (size_t)index * rq::RQ_PACKED_FLOATS, image.data(), (size_t)rq::RQ_PACKED_FLOATS * sizeof(float), hipMemcpyHostToDevice));
    RQ_HIP(hipMemcpy(bank->weights + (size_t)index * RQ_POLICY_NUM_WEIGHTS, weights, RQ_POLICY_NUM_WEIGHTS * sizeof(float), hipMemcpyHostToDevice));
    return RQ_OK;
}

}  // namespace

extern "C" {

RQ_API int rq_policy_bank_create(rq_device* dev, const float* weights, uint32_t n_policies, rq_policy_bank** out) {
    RQ_REQUIRE(dev && weights && out, RQ_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    RQ_REQUIRE(n_policies > 0, RQ_ERR_INVALID_ARGUMENT, "n_policies must be positive");
    DeviceScope on_device(dev); int rc = on_device.rc; if (rc) return rc;
    rq_policy_bank* b = new (std::nothrow) rq_policy_bank();
    RQ_REQUIRE(b, RQ_ERR_OUT_OF_MEMORY, "host allocation failed");
    b->dev = dev; b->ordinal = dev->ordinal; b->n_policies = n_policies;
    std::vector<float> images;
    try { images.resize((size_t)rq::RQ_PACKED_FLOATS * n_policies); } catch (const std::bad_alloc&) {
        delete b;
        return fail(RQ_ERR_OUT_OF_MEMORY, "rq_policy_bank_create: host allocation failed");
    }
    for (uint32_t k = 0; k < n_policies; ++k)
        rq::pack_policy(weights + (size_t)k * RQ_POLICY_NUM_WEIGHTS, images.data() + (size_t)k * rq::RQ_PACKED_FLOATS);
    try { b->intervals.assign(n_policies, 1u); } catch (const std::bad_alloc&) {
        delete b;
        return fail(RQ_ERR_OUT_OF_MEMORY, "rq_policy_bank_create: host allocation failed");
    }
    const size_t raw = (size_t)RQ_POLICY_NUM_WEIGHTS * n_policies;
    if (b->images.alloc(images.size()) != hipSuccess || b->weights.alloc(raw) != hipSuccess ||
        b->intervals_dev.alloc(n_policies) != hipSuccess ||
        hipMemcpy(b->images, images.data(), images.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(b->weights, weights, raw * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(b->intervals_dev, b->intervals.data(), (size_t)n_policies * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
        delete b;
        return fail(RQ_ERR_OUT_OF_MEMORY, "rq_policy_bank_create: device allocation or upload failed");
    }
    policy_bank_registry(b, +1);
    *out = b;
    return RQ_OK;
}

RQ_API int rq_policy_bank_destroy(rq_policy_bank* bank) {
    if (!bank) return RQ_OK;
    DeviceScope on_device(bank->ordinal);      // (hipFree synchronises the device: no launch still reads the images)
    policy_bank_registry(bank, -1);            // an optimizer may still name this object: it is checked against the registry
    delete bank;
    return RQ_OK;
}

RQ_API int rq_policy_bank_set_weights(rq_policy_bank* bank, uint32_t index, const float* weights) {
    RQ_REQUIRE(bank && weights, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(index < bank->n_policies, RQ_ERR_INVALID_ARGUMENT,
               "policy index " + std::to_string(index) + " is outside a bank of " + std::to_string(bank->n_policies) + " (" + kWeightsShape + ")");
    DeviceScope on_device(bank->dev); int rc = on_device.rc; if (rc) return rc;
    RQ_HIP(hipStreamSynchronize(bank->dev->stream));          // a rollout in flight reads the slot
    return bank_upload_slot(bank, index, weights);
}

RQ_API int rq_policy_bank_get_weights(rq_policy_bank* bank, float* out) {
    RQ_REQUIRE(bank && out, RQ_ERR_INVALID_ARGUMENT, "null argument");
    DeviceScope on_device(bank->dev); int rc = on_device.rc; if (rc) return rc;
    RQ_HIP(hipMemcpyAsync(out, bank->weights, (size_t)bank->n_policies * RQ_POLICY_NUM_WEIGHTS * sizeof(float), hipMemcpyDeviceToHost,
                          bank->dev->stream));              // behind every update enqueued so far
    RQ_HIP(hipStreamSynchronize(bank->dev->stream));
    return RQ_OK;
}

RQ_API int rq_policy_bank_set_native_interval(rq_policy_bank* bank, const uint32_t* interval, uint32_t n) {
    RQ_REQUIRE(bank && interval, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(n == 1 || n == bank->n_policies, RQ_ERR_INVALID_ARGUMENT,
               "n must be 1 (one interval for every policy) or the bank's " + std::to_string(bank->n_policies) + " policies, not " + std::to_string(n));
    for (uint32_t k = 0; k < n; ++k)
        RQ_REQUIRE(interval[k] >= 1 && interval[k] <= RQ_POLICY_MAX_NATIVE_INTERVAL, RQ_ERR_INVALID_ARGUMENT,
                   "native interval must be 1 .. " + std::to_string(RQ_POLICY_MAX_NATIVE_INTERVAL) + ": interval[" + std::to_string(k) + "] is " +
                       std::to_string(interval[k]));
    DeviceScope on_device(bank->dev); int rc = on_device.rc; if (rc) return rc;
    RQ_HIP(hipStreamSynchronize(bank->dev->stream));          // a rollout in flight reads the table
    std::vector<uint32_t> table;
    try { table.resize(bank->n_policies); } catch (const std::bad_alloc&) {
        return fail(RQ_ERR_OUT_OF_MEMORY, "policy bank: host allocation failed");
    }
    bool rated = false;
    for (uint32_t p = 0; p < bank->n_policies; ++p) { table[p] = interval[n == 1 ? 0 : p]; rated = rated || table[p] > 1; }
    // (synchronous: the caller's array is its own again on return; the host's copy changes only with the device's)
    RQ_HIP(hipMemcpy(bank->intervals_dev, table.data(), table.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    bank->intervals.swap(table);
    bank->rated = rated;
    return RQ_OK;
}

RQ_API int rq_policy_bank_get_native_interval(const rq_policy_bank* bank, uint32_t* out) {
    RQ_REQUIRE(bank && out, RQ_ERR_INVALID_ARGUMENT, "null argument");
    std::memcpy(out, bank->intervals.data(), (size_t)bank->n_policies * sizeof(uint32_t));
    return RQ_OK;
}

RQ_API int rq_policy_bank_reset(rq_policy_bank* bank) {
    RQ_REQUIRE(bank, RQ_ERR_INVALID_ARGUMENT, "null argument");
    bank->needs_reset = true;      // applied on the next use, when the assignment says whose initial state an env takes
    return RQ_OK;
}

RQ_API int rq_policy_bank_get_hidden(rq_policy_bank* bank, float* host_out, uint32_t batch) {
    RQ_REQUIRE(bank && host_out, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(bank->hidden && bank->table_valid, RQ_ERR_NOT_INITIALIZED,
               "the hidden state is sized, and its initial value chosen per env, by the first rq_rollout_policies");
    RQ_REQUIRE(batch == bank->batch && bank->table_ids.size() == blocks_of(batch), RQ_ERR_SHAPE_MISMATCH,
               "batch does not match the envs this bank last flew");
    DeviceScope on_device(bank->dev); int rc = on_device.rc; if (rc) return rc;
    rc = bank_apply_reset(bank); if (rc) return rc;
    return soa_to_host(bank->dev, bank->hidden, batch, bank->ld, RQ_POLICY_HIDDEN_DIM, host_out);
}

}  // extern "C"

namespace {

// A bank's policies fly the envs by policy_id, plain launches when chained.  With every interval 1 the launches are the ones a
// bank's rollout always made; otherwise the RATE kernels (fused: rq_fused_route.hpp).
struct PolicyBankActor {
    static constexpr bool kFoldAndReplay = false;
    rq_policy_bank* bank; const uint32_t* policy_id;
    bool given() const { return bank && policy_id; }
    int check(const RolloutCall& c, const RolloutFrame&) const {
        RQ_REFUSE(c.who, bank->dev == c.dev, RQ_ERR_SHAPE_MISMATCH, "policy bank lives on another device");
        return bank_check_ids(bank, policy_id, c.env->n);
    }
    int prepare(const RolloutCall& c) const {
        int rc = bank_size(bank, c.env->n); if (rc) return rc;
        RQ_REFUSE(c.who, bank->ld == c.env->ld, RQ_ERR_SHAPE_MISMATCH, "policy bank batch does not match the env");
        rc = bank_table(bank, c.dev, c.env->uid, policy_id, c.env->n); if (rc) return rc;
        return bank_apply_reset(bank);
    }
    int fused(const RolloutCall& c, const RolloutFrame& f) const {
        rq::FusedArgs a = fused_args(c, f);
        a.hidden = bank->hidden; a.weights = bank->weights;
        a.images = bank->images; a.block_policy = bank->table; a.policy_interval = bank->intervals_dev; a.bank_rated = bank->rated;
        return fused_launch(c, a);
    }
    rq::EnvStepLaunch env_step(const RolloutCall& c, const RolloutFrame& f) const {
        rq::EnvStepLaunch e = env_step_launch(c, f);
        e.hidden = bank->hidden; e.weights = bank->weights; e.block_policy = bank->table;
        return e;
    }
    hipError_t thaw(const RolloutCall& c, const RolloutFrame& f) const { return rq::launch_thaw_frozen(c.dev->stream, env_step(c, f)); }
    hipError_t act(const RolloutCall& c, const RolloutFrame&, uint32_t, const uint32_t*) const {
        const rq_env* env = c.env;
        rq::ActorStepLaunch a;
        a.n = env->n; a.images = bank->images; a.block_policy = bank->table; a.policy_interval = bank->rated ? bank->intervals_dev.get() : nullptr;
        a.obs = env->obs; a.ld_obs = env->ld; a.hidden = bank->hidden; a.ld_h = bank->ld; a.act = env->act; a.ld_act = env->ld;
        a.frozen = env->st.frozen; a.steps = env->st.steps;
        return rq::launch_actor_step(c.dev->stream, a);
    }
    hipError_t step(const RolloutCall& c, const RolloutFrame& f, uint32_t, const uint32_t*, bool) const {
        return rq::launch_step(c.dev->stream, env_step(c, f));
    }
};

}  // namespace

extern "C" {

RQ_API int rq_rollout_policies(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state, rq_policy_bank* bank,
                               const uint32_t* policy_id, rq_rng* rng, uint32_t n_steps, int mode, uint32_t flags,
                               rq_trajectory* traj) {
    return rollout_run({__func__, dev, env, params, state, rng, n_steps, mode, flags, traj, nullptr, nullptr},
                       PolicyBankActor{bank, policy_id});
}

RQ_API int rq_rollout_policies_track(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state, rq_policy_bank* bank,
                                     const uint32_t* policy_id, rq_rng* rng, uint32_t n_steps, int mode, uint32_t flags,
                                     rq_trajectory* traj, const rq_reference* reference) {
    RQ_REQUIRE(reference, RQ_ERR_INVALID_ARGUMENT, "null reference");
    return rollout_run({__func__, dev, env, params, state, rng, n_steps, mode, flags, traj, reference, nullptr},
                       PolicyBankActor{bank, policy_id});
}

RQ_API int rq_rollout_policies_track_refs(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state, rq_policy_bank* bank,
                                          const uint32_t* policy_id, rq_rng* rng, uint32_t n_steps, int mode, uint32_t flags,
                                          rq_trajectory* traj, const rq_reference_bank* references, const uint32_t* reference_id) {
    RQ_REQUIRE(references, RQ_ERR_INVALID_ARGUMENT, "null reference bank");
    RQ_REQUIRE(reference_id, RQ_ERR_INVALID_ARGUMENT, "null reference_id");
    return rollout_run({__func__, dev, env, params, state, rng, n_steps, mode, flags, traj, references, reference_id},
                       PolicyBankActor{bank, policy_id});
}

}  // extern "C"
