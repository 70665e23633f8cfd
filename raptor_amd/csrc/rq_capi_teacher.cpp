// rq_capi_teacher.cpp - the teacher bank: the distillation step of the reference (README.md:208-216: ~1000 MLP teachers queried on
// student-visited states), register-stationary family and dense stacks (rq_teacher.hip).
#include "rq_objects.hpp"

using namespace rqh;

// what both constructors refuse
static int check_bank_args(uint32_t n_teachers, uint32_t in_dim, int hidden_activation, int output_activation) {
    RQ_REQUIRE(n_teachers > 0, RQ_ERR_INVALID_ARGUMENT, "n_teachers must be positive");
    RQ_REQUIRE(in_dim >= 1 && in_dim <= RQ_POLICY_INPUT_DIM, RQ_ERR_INVALID_ARGUMENT,
               "in_dim must be 1..22 (the recorded policy inputs)");
    RQ_REQUIRE(hidden_activation == RQ_ACT_RELU || hidden_activation == RQ_ACT_TANH, RQ_ERR_INVALID_ARGUMENT,
               "hidden activation must be RQ_ACT_RELU or RQ_ACT_TANH");
    RQ_REQUIRE(output_activation == RQ_ACT_IDENTITY || output_activation == RQ_ACT_TANH, RQ_ERR_INVALID_ARGUMENT,
               "output activation must be RQ_ACT_IDENTITY or RQ_ACT_TANH");
    return RQ_OK;
}

// the image, allocated and uploaded
static hipError_t upload(DeviceBuffer<float>& dst, const std::vector<float>& image) {
    const hipError_t e = dst.alloc(image.size());
    return e != hipSuccess ? e : hipMemcpy(dst, image.data(), image.size() * sizeof(float), hipMemcpyHostToDevice);
}

extern "C" {

// ---------------------------------------------------------------------------- Teacher bank
RQ_API int rq_teacher_bank_create(rq_device* dev, const float* weights, uint32_t n_teachers, uint32_t in_dim, uint32_t h1,
                           uint32_t h2, int hidden_activation, int output_activation, rq_teacher_bank** out) {
    RQ_REQUIRE(dev && weights && out, RQ_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    auto ok_width = [](uint32_t h) { return h == 16 || h == 32 || h == 64; };
    RQ_REQUIRE(ok_width(h1) && ok_width(h2), RQ_ERR_INVALID_ARGUMENT, "hidden widths must be 16, 32 or 64");
    int rc = check_bank_args(n_teachers, in_dim, hidden_activation, output_activation); if (rc) return rc;
    DeviceScope on_device(dev); rc = on_device.rc; if (rc) return rc;
    rq_teacher_bank* b = new (std::nothrow) rq_teacher_bank();
    RQ_REQUIRE(b, RQ_ERR_OUT_OF_MEMORY, "host allocation failed");
    b->dev = dev; b->ordinal = dev->ordinal; b->n_teachers = n_teachers; b->in_dim = in_dim; b->h1 = h1; b->h2 = h2;
    b->act = hidden_activation; b->out_act = output_activation;
    const size_t per = rq::teacher_param_count((int)in_dim, (int)h1, (int)h2);
    const size_t f32_floats = (size_t)rq::teacher_image_regs_f32((int)h1, (int)h2) * 64;
    const size_t bf16_floats = (size_t)rq::teacher_image_regs_bf16((int)h1, (int)h2) * 64;
    const size_t split_floats = (size_t)rq::teacher_image_regs_f16x2((int)h1, (int)h2) * 64;
    std::vector<float> img32, img16, img_split;
    try {                                   // nothing throws across the boundary
        img32.resize(f32_floats * n_teachers);
        img16.resize(bf16_floats * n_teachers);
        img_split.resize(split_floats * n_teachers);
    } catch (const std::bad_alloc&) {
        delete b;
        return fail(RQ_ERR_OUT_OF_MEMORY, "rq_teacher_bank_create: host allocation failed");
    }
    for (uint32_t t = 0; t < n_teachers; ++t) {
        rq::pack_teacher_f32(weights + per * t, (int)in_dim, (int)h1, (int)h2, b->act, b->out_act, img32.data() + f32_floats * t);
        rq::pack_teacher_bf16(weights + per * t, (int)in_dim, (int)h1, (int)h2, b->act, b->out_act, img16.data() + bf16_floats * t);
        if (!rq::pack_teacher_f16x2(weights + per * t, (int)in_dim, (int)h1, (int)h2, b->act, b->out_act, img_split.data() + split_floats * t) &&
            b->f16x2_misfit == UINT32_MAX)
            b->f16x2_misfit = t;
    }
    if (upload(b->images_f32, img32) != hipSuccess || upload(b->images_bf16, img16) != hipSuccess ||
        upload(b->images_f16x2, img_split) != hipSuccess) {
        delete b;
        return fail(RQ_ERR_OUT_OF_MEMORY, "rq_teacher_bank_create: device allocation or upload failed");
    }
    *out = b;
    return RQ_OK;
}

RQ_API int rq_teacher_bank_create_layers(rq_device* dev, const float* weights, uint32_t n_teachers, uint32_t in_dim, uint32_t n_hidden,
                                  const uint32_t* widths, int hidden_activation, int output_activation, rq_teacher_bank** out) {
    RQ_REQUIRE(dev && weights && widths && out, RQ_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    RQ_REQUIRE(n_hidden >= 1 && n_hidden <= 3, RQ_ERR_INVALID_ARGUMENT, "a teacher has one, two or three hidden layers");
    auto fast_width = [](uint32_t h) { return h == 16 || h == 32 || h == 64; };
    if (n_hidden == 2 && fast_width(widths[0]) && fast_width(widths[1]))      // the register-stationary family (three precisions)
        return rq_teacher_bank_create(dev, weights, n_teachers, in_dim, widths[0], widths[1], hidden_activation, output_activation, out);
    uint32_t widest = 0;
    for (uint32_t l = 0; l < n_hidden; ++l) {
        RQ_REQUIRE(widths[l] >= 16 && widths[l] <= 128 && widths[l] % 16 == 0, RQ_ERR_INVALID_ARGUMENT,
                   "hidden widths must be multiples of 16 from 16 to 128");
        widest = widths[l] > widest ? widths[l] : widest;
    }
    int rc = check_bank_args(n_teachers, in_dim, hidden_activation, output_activation); if (rc) return rc;
    DeviceScope on_device(dev); rc = on_device.rc; if (rc) return rc;
    rq_teacher_bank* b = new (std::nothrow) rq_teacher_bank();
    RQ_REQUIRE(b, RQ_ERR_OUT_OF_MEMORY, "host allocation failed");
    b->dev = dev; b->ordinal = dev->ordinal; b->n_teachers = n_teachers; b->in_dim = in_dim;
    b->act = hidden_activation; b->out_act = output_activation;
    b->layers = true; b->n_hidden = n_hidden; b->hp = widest <= 64 ? 64u : 128u;
    for (uint32_t l = 0; l < n_hidden; ++l) b->widths[l] = widths[l];
    b->h1 = widths[0]; b->h2 = n_hidden > 1 ? widths[1] : 0;
    const size_t per = rq::teacher_layers_param_count((int)in_dim, (int)n_hidden, widths);
    const size_t floats = rq::teacher_layers_image_floats((int)b->hp, (int)n_hidden);
    std::vector<float> img;
    try {                                   // nothing throws across the boundary
        img.resize(floats * n_teachers);
    } catch (const std::bad_alloc&) {
        delete b;
        return fail(RQ_ERR_OUT_OF_MEMORY, "rq_teacher_bank_create_layers: host allocation failed");
    }
    for (uint32_t t = 0; t < n_teachers; ++t)
        rq::pack_teacher_layers(weights + per * t, (int)in_dim, (int)n_hidden, widths, (int)b->hp, b->act, b->out_act, img.data() + floats * t);
    if (upload(b->images_layers, img) != hipSuccess) {
        delete b;
        return fail(RQ_ERR_OUT_OF_MEMORY, "rq_teacher_bank_create_layers: device allocation or upload failed");
    }
    *out = b;
    return RQ_OK;
}

RQ_API int rq_teacher_bank_destroy(rq_teacher_bank* bank) {
    if (!bank) return RQ_OK;
    DeviceScope on_device(bank->ordinal);
    delete bank;
    return RQ_OK;
}

RQ_API int rq_teacher_bank_set_precision(rq_teacher_bank* bank, int precision) {
    RQ_REQUIRE(bank, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(precision == RQ_POLICY_FP32 || precision == RQ_POLICY_BF16_MFMA || precision == RQ_POLICY_F16X2_MFMA,
               RQ_ERR_INVALID_ARGUMENT, "unknown precision");
    RQ_REQUIRE(!bank->layers || precision == RQ_POLICY_FP32, RQ_ERR_INVALID_ARGUMENT,
               "a bank outside the two-hidden-layer {16, 32, 64} family is evaluated in fp32 only");
    if (precision == RQ_POLICY_F16X2_MFMA && bank->f16x2_misfit != UINT32_MAX) {
        char msg[200];
        std::snprintf(msg, sizeof msg, "teacher %u has a weight outside the f16 range (|w| >= 65520 after the tanh pre-scale of "
                      "-2 log2 e): the f16x2 image cannot hold it, use fp32 or bf16", bank->f16x2_misfit);
        return fail(RQ_ERR_INVALID_ARGUMENT, msg);
    }
    bank->precision = precision;
    return RQ_OK;
}

}  // extern "C"

namespace {

// teacher_id[0..n) all name a teacher of the bank (checked before anything is enqueued)
int check_ids(const rq_teacher_bank* bank, const uint32_t* teacher_id, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i)
        RQ_REQUIRE(teacher_id[i] < bank->n_teachers, RQ_ERR_INVALID_ARGUMENT, "teacher id out of range");
    return RQ_OK;
}

// The bank's device tile list for n envs assigned by teacher_id, built and uploaded only when (key, ids) differ from what `tiles`
// holds - a loop of rollout chunks or relabels with one assignment pays no copy and no stream synchronisation after its first call.
// Group the envs by teacher: register-stationary family: tile_teacher [n_tiles] | tile_env [n_tiles][16] (a tile = up to 16 envs of
// ONE teacher, counting sort over the ids, env order kept inside a teacher, so sorted inputs give contiguous tiles and coalesced rows);
// dense stacks (round 6): teacher_start [n_teachers + 1] | sorted_env [n] - the kernel forms its 16-wide tiles out of (env, step) pairs.
// Needs the caller's DeviceScope.
int bank_tiles(rq_teacher_bank* bank, rq_device* dev, uint64_t key, const uint32_t* teacher_id, uint32_t n, uint32_t* n_tiles_out) {
    if (bank->tiles_valid && bank->tiles_key == key && bank->tiles_ids.size() == n &&
        std::memcmp(bank->tiles_ids.data(), teacher_id, (size_t)n * sizeof(uint32_t)) == 0) {
        *n_tiles_out = bank->tiles_count;
        return RQ_OK;
    }
    std::vector<uint32_t> host;
    uint32_t n_tiles = 0;
    try {                                   // nothing throws across the boundary
        std::vector<uint32_t> count(bank->n_teachers, 0), start(bank->n_teachers, 0), filled(bank->n_teachers, 0);
        for (uint32_t i = 0; i < n; ++i) ++count[teacher_id[i]];
        if (bank->layers) {
            host.assign((size_t)bank->n_teachers + 1 + n, 0u);
            uint32_t at = 0;
            for (uint32_t k = 0; k < bank->n_teachers; ++k) { host[k] = start[k] = at; at += count[k]; }
            host[bank->n_teachers] = at;
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t k = teacher_id[i];
                host[(size_t)bank->n_teachers + 1 + start[k] + filled[k]++] = i;
            }
        } else {
            for (uint32_t k = 0; k < bank->n_teachers; ++k) { start[k] = n_tiles; n_tiles += (count[k] + 15u) / 16u; }
            host.assign((size_t)n_tiles * 17, 0xFFFFFFFFu);
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t k = teacher_id[i], pos = filled[k]++;
                const uint32_t tile = start[k] + pos / 16u;
                host[tile] = k;
                host[(size_t)n_tiles + (size_t)tile * 16 + pos % 16u] = i;
            }
        }
        bank->tiles_valid = false;
        bank->tiles_ids.assign(teacher_id, teacher_id + n);
    } catch (const std::bad_alloc&) {
        return fail(RQ_ERR_OUT_OF_MEMORY, "teacher bank: host allocation failed");
    }
    RQ_HIP(bank->tiles.reserve(dev->stream, host.size()));
    RQ_HIP(hipMemcpyAsync(bank->tiles, host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice, dev->stream));
    RQ_HIP(hipStreamSynchronize(dev->stream));                // `host` is pageable and about to go out of scope
    bank->tiles_valid = true;
    bank->tiles_key = key;
    bank->tiles_count = n_tiles;
    *n_tiles_out = n_tiles;
    return RQ_OK;
}

// bank_label's launch alone (any kind, any precision), for callers that report a failure themselves (rollout_chained)
hipError_t bank_label_launch(rq_teacher_bank* bank, rq_device* dev, uint32_t n, uint32_t n_tiles, uint32_t ld, uint32_t steps,
                             const float* obs, float* act) {
    const float* images = bank->precision == RQ_POLICY_BF16_MFMA ? bank->images_bf16
                        : bank->precision == RQ_POLICY_F16X2_MFMA ? bank->images_f16x2 : bank->images_f32;
    if (bank->layers)
        return rq::launch_teacher_relabel_layers(dev->stream, bank->n_teachers, n, ld, steps, bank->in_dim, bank->n_hidden, bank->hp,
                                                 bank->act, bank->out_act, bank->images_layers, bank->tiles, bank->tiles + bank->n_teachers + 1,
                                                 obs, act);
    return rq::launch_teacher_relabel(dev->stream, n_tiles, ld, steps, bank->in_dim, bank->h1, bank->h2, bank->act, bank->out_act,
                                      bank->precision, images, bank->tiles, bank->tiles + n_tiles, obs, act);
}
// the bank's actions on obs [steps][22][ld] -> act [steps][4][ld] for the n envs of the tile list bank_tiles made (any kind, any precision)
int bank_label(rq_teacher_bank* bank, rq_device* dev, uint32_t n, uint32_t n_tiles, uint32_t ld, uint32_t steps, const float* obs,
               float* act) {
    RQ_HIP(bank_label_launch(bank, dev, n, n_tiles, ld, steps, obs, act));
    return RQ_OK;
}

}  // namespace

extern "C" {

RQ_API int rq_trajectory_relabel_teachers(rq_trajectory* t, rq_teacher_bank* bank, const uint32_t* teacher_id, float* action_out,
                                   int overwrite) {
    RQ_REQUIRE(t && bank && teacher_id, RQ_ERR_INVALID_ARGUMENT, "null argument");
    rq_env* env = t->env;
    rq_device* dev = env->dev;
    RQ_REQUIRE(bank->dev == dev, RQ_ERR_SHAPE_MISMATCH, "teacher bank lives on another device");
    if (t->length == 0) return RQ_OK;
    const uint32_t n = env->n;
    int rc = check_ids(bank, teacher_id, n); if (rc) return rc;
    if (bank->layers)
        RQ_REQUIRE((uint64_t)n * t->length < (1ull << 32), RQ_ERR_INVALID_ARGUMENT, "envs x steps must stay below 2^32 for a dense-stack bank");
    DeviceScope on_device(dev); rc = on_device.rc; if (rc) return rc;
    uint32_t n_tiles = 0;
    rc = bank_tiles(bank, dev, env->uid, teacher_id, n, &n_tiles); if (rc) return rc;
    float* d_act = t->act;
    if (!overwrite) {
        RQ_HIP(dev->rows2.reserve(dev->stream, (size_t)t->length * RQ_ACTION_DIM * env->ld));
        d_act = dev->rows2;
    }
    rc = bank_label(bank, dev, n, n_tiles, env->ld, t->length, t->obs, d_act); if (rc) return rc;
    if (action_out) return traj_block_to_host(dev, d_act, t->length, env->n, env->ld, RQ_ACTION_DIM, action_out);
    return RQ_OK;
}

RQ_API int rq_teacher_bank_evaluate(rq_teacher_bank* bank, rq_env* env, const uint32_t* teacher_id, const float* observation,
                                    uint32_t batch, uint32_t obs_stride, float* action) {
    RQ_REQUIRE(bank && teacher_id, RQ_ERR_INVALID_ARGUMENT, "null argument");
    const bool on_env = observation == nullptr || action == nullptr;          // reads or writes the env's device buffers
    RQ_REQUIRE(env || !on_env, RQ_ERR_INVALID_ARGUMENT, "a NULL observation / action names the env's device buffer: env is required");
    rq_device* dev = bank->dev;
    if (env) {
        RQ_REQUIRE(env->dev == dev, RQ_ERR_SHAPE_MISMATCH, "env lives on another device than the teacher bank");
        RQ_REQUIRE(env->initialized, RQ_ERR_NOT_INITIALIZED, "initialize_environment was not called");
    }
    RQ_REQUIRE(batch > 0, RQ_ERR_INVALID_ARGUMENT, "batch must be positive");
    if (on_env) RQ_REQUIRE(batch == env->n, RQ_ERR_SHAPE_MISMATCH, "the env's buffers hold N_ENVIRONMENTS rows: batch must equal it");
    if (observation) RQ_REQUIRE(obs_stride >= bank->in_dim, RQ_ERR_INVALID_ARGUMENT, "obs_stride is below the teachers' input width");
    int rc = check_ids(bank, teacher_id, batch); if (rc) return rc;
    DeviceScope on_device(dev); rc = on_device.rc; if (rc) return rc;
    const uint32_t ld = on_env ? env->ld : round_up64(batch);
    uint32_t n_tiles = 0;
    rc = bank_tiles(bank, dev, on_env ? env->uid : 0, teacher_id, batch, &n_tiles); if (rc) return rc;
    const float* d_obs = on_env && !observation ? env->obs : nullptr;
    float* d_act = action ? nullptr : env->act;
    if (observation || action) {
        const size_t rows = observation ? (size_t)batch * obs_stride : 0;
        RQ_HIP(bank->eval_buf.reserve(dev->stream, rows + (size_t)(RQ_POLICY_INPUT_DIM + RQ_ACTION_DIM) * ld));
        if (observation) {
            float* soa = bank->eval_buf + rows;
            RQ_HIP(hipMemcpyAsync(bank->eval_buf, observation, rows * sizeof(float), hipMemcpyHostToDevice, dev->stream));
            RQ_HIP(rq::launch_rows_to_soa(dev->stream, bank->eval_buf, obs_stride, std::min<uint32_t>(obs_stride, RQ_POLICY_INPUT_DIM),
                                          batch, ld, soa));
            d_obs = soa;
        }
        if (action) d_act = bank->eval_buf + rows + (size_t)RQ_POLICY_INPUT_DIM * ld;
    }
    if (!action) obs_cache_drop_if(dev, env);
    rc = bank_label(bank, dev, batch, n_tiles, ld, 1, d_obs, d_act); if (rc) return rc;
    if (action) return traj_block_to_host(dev, d_act, 1, batch, ld, RQ_ACTION_DIM, action);
    RQ_HIP(hipStreamSynchronize(dev->stream));                // the host rows are read before the call returns
    return RQ_OK;
}

}  // extern "C"

namespace {

// The bank's teachers fly the envs by teacher_id, plain launches when chained: the actor is the bank on the env's buffers
// (rq_teacher_bank_evaluate's launch).  k_step's auto-reset also resets a policy state: a teacher has none, so it writes the
// bank's sink (a zero weight block and a [16][ld] target).
struct TeacherActor {
    static constexpr bool kFoldAndReplay = false;
    rq_teacher_bank* bank; const uint32_t* teacher_id;
    uint32_t n_tiles = 0;
    bool given() const { return bank && teacher_id; }
    float* sink_w() const { return bank->sink; }
    float* sink_h() const { return bank->sink + RQ_POLICY_NUM_WEIGHTS; }
    int check(const RolloutCall& c, const RolloutFrame& f) const {
        RQ_REFUSE(c.who, bank->dev == c.dev, RQ_ERR_SHAPE_MISMATCH, "teacher bank lives on another device");
        RQ_REFUSE(c.who, c.mode != RQ_ROLLOUT_FUSED || (!bank->layers && bank->precision == RQ_POLICY_FP32), RQ_ERR_INVALID_ARGUMENT,
                  "the fused teacher rollout runs the fp32 two-hidden-layer {16, 32, 64} family: fly this bank (bf16 / f16x2 precision "
                  "or a dense stack) with mode RQ_ROLLOUT_CHAINED (\"chained\")");
        for (int k = 0; k < kScheduleKinds && c.mode == RQ_ROLLOUT_FUSED; ++k)
            if (f.sched[k].rows) return refuses_fused(c.who, k, "a teacher bank");
        return check_ids(bank, teacher_id, c.env->n);
    }
    int prepare(const RolloutCall& c) {
        const int rc = bank_tiles(bank, c.dev, c.env->uid, teacher_id, c.env->n, &n_tiles); if (rc) return rc;
        if (c.mode == RQ_ROLLOUT_CHAINED && c.n_steps) {
            RQ_HIP(bank->sink.reserve(c.dev->stream, RQ_POLICY_NUM_WEIGHTS + (size_t)16 * c.env->ld));
            RQ_HIP(hipMemsetAsync(sink_w(), 0, RQ_POLICY_NUM_WEIGHTS * sizeof(float), c.dev->stream));
        }
        return RQ_OK;
    }
    int fused(const RolloutCall& c, const RolloutFrame& f) const {
        rq::TeacherRolloutArgs a{f.b, f.sc, f.nc, f.smp, c.rng->seed, c.rng->epoch, c.n_steps, f.noise ? 1u : 0u,
                                 (c.flags & RQ_ROLLOUT_AUTORESET) ? 1u : 0u, c.params->d, c.state->d, c.env->st, f.tp,
                                 bank->in_dim, bank->images_f32, bank->tiles, bank->tiles + n_tiles, f.trk};
        RQ_HIP(rq::launch_rollout_teachers(c.dev->stream, n_tiles, bank->h1, bank->h2, bank->act, bank->out_act, a));
        return RQ_OK;
    }
    rq::EnvStepLaunch env_step(const RolloutCall& c, const RolloutFrame& f) const {
        rq::EnvStepLaunch e = env_step_launch(c, f);
        e.hidden = sink_h(); e.weights = sink_w();
        return e;
    }
    hipError_t thaw(const RolloutCall& c, const RolloutFrame& f) const { return rq::launch_thaw_frozen(c.dev->stream, env_step(c, f)); }
    hipError_t act(const RolloutCall& c, const RolloutFrame&, uint32_t, const uint32_t*) const {
        return bank_label_launch(bank, c.dev, c.env->n, n_tiles, c.env->ld, 1, c.env->obs, c.env->act);
    }
    hipError_t step(const RolloutCall& c, const RolloutFrame& f, uint32_t, const uint32_t*, bool) const {
        return rq::launch_step(c.dev->stream, env_step(c, f));
    }
};

}  // namespace

extern "C" {

RQ_API int rq_rollout_teachers(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state, rq_teacher_bank* bank,
                               const uint32_t* teacher_id, rq_rng* rng, uint32_t n_steps, int mode, uint32_t flags,
                               rq_trajectory* traj) {
    return rollout_run({__func__, dev, env, params, state, rng, n_steps, mode, flags, traj, nullptr, nullptr},
                       TeacherActor{bank, teacher_id});
}

RQ_API int rq_rollout_teachers_track(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state, rq_teacher_bank* bank,
                                     const uint32_t* teacher_id, rq_rng* rng, uint32_t n_steps, int mode, uint32_t flags,
                                     rq_trajectory* traj, const rq_reference* reference) {
    RQ_REQUIRE(reference, RQ_ERR_INVALID_ARGUMENT, "null reference");
    return rollout_run({__func__, dev, env, params, state, rng, n_steps, mode, flags, traj, reference, nullptr},
                       TeacherActor{bank, teacher_id});
}

RQ_API int rq_rollout_teachers_track_refs(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state, rq_teacher_bank* bank,
                                          const uint32_t* teacher_id, rq_rng* rng, uint32_t n_steps, int mode, uint32_t flags,
                                          rq_trajectory* traj, const rq_reference_bank* references, const uint32_t* reference_id) {
    RQ_REQUIRE(references, RQ_ERR_INVALID_ARGUMENT, "null reference bank");
    RQ_REQUIRE(reference_id, RQ_ERR_INVALID_ARGUMENT, "null reference_id");
    return rollout_run({__func__, dev, env, params, state, rng, n_steps, mode, flags, traj, references, reference_id},
                       TeacherActor{bank, teacher_id});
}

}  // extern "C"
