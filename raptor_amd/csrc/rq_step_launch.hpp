// rq_step_launch.hpp - what one launch of the chained step's kernels is: the actor step (ActorStepLaunch; launch_actor_step,
// rq_kernels.hip, reads it) and the env step with its thaw (EnvStepLaunch; launch_step, launch_thaw_frozen), as rq_step,
// rq_policy_evaluate_step, the small-batch loop and the chained rollouts fill them - and which kernel serves an actor step
// (route_actor_step: the one statement of that choice; the launcher switches on its answer).  Host code without a HIP dependency: a
// plain host compiler takes this file alone (tests/actor_step_route_driver.cpp does, and holds every row of the route against
// tests/test_capi_cpu.py's own table).
#pragma once
#include <stdint.h>

#include "../../include/raptor_quad.h"

namespace rq {

// ---- the argument blocks the kernels take by value (they land in SGPRs via the kernarg segment) -----------------------------------
struct StepCfg {   // the rq_env_config members one transition reads
    float dt, gravity;
    uint32_t episode_step_limit;
    float reward_scale, reward_constant, reward_termination_penalty;
    float reward_position, reward_orientation, reward_linear_velocity, reward_angular_velocity, reward_action;
    uint32_t termination_enabled;
    float termination_position, termination_linear_velocity, termination_angular_velocity;
    uint32_t action_history_raw;
};

struct NoiseCfg { float position, orientation, linear_velocity, angular_velocity; };

struct SampleCfg {   // rq_env_config members the samplers read
    float gravity;
    uint32_t domain_randomization;
    float dr_scale_min, dr_scale_max, dr_t2w_min, dr_t2w_max, dr_kq_min, dr_kq_max, dr_tau_min, dr_tau_max;
    float init_guidance, init_max_position, init_max_angle, init_max_linear_velocity, init_max_angular_velocity;
    float disturbance_force_std, disturbance_torque_std;
};

// Episode statistics of one VectorEnvironment, all [ld] arrays on the device.
struct StatsPtrs {
    float* returns; uint32_t* steps;
    float* fin_returns; uint32_t* fin_lengths; uint32_t* fin_counts; uint32_t* fin_terminated;
    float* last_reward; uint8_t* last_terminated;
    uint8_t* frozen; uint32_t* episode;
    uint8_t* last_done;   // per transition: 0 running, 1 terminated, 2 step limit reached, 4 env frozen (not stepped)
};

// A wrench schedule (rq_env_set_wrench_schedule): the bank's tables and the env's per-env first rows (rq_device_math.hpp wrench_*).
struct WrenchPtrs {
    const float* rows;        // [n_tables * n_rows][6] row-major: force (world frame), torque (body frame); nullptr = no schedule
    const uint32_t* row0;     // [ld]: wrench_id[i] * n_rows, the first row of env i's table
    uint32_t n_rows;          // rows of one table
    uint32_t relative;        // 1: multiples of m g / m g arm (RQ_WRENCH_RELATIVE); 0: N / N m
};

// A vehicle schedule (rq_env_set_vehicle_schedule): the bank's tables and the env's per-env first rows (rq_device_math.hpp vehicle_*).
struct VehiclePtrs {
    const float* rows;        // [n_tables * n_rows][4] row-major: factors on mass, inertia, thrust, motor time constant; nullptr = none
    const uint32_t* row0;     // [ld]: vehicle_id[i] * n_rows, the first row of env i's table
    uint32_t n_rows;          // rows of one table
    uint32_t pad_;
};

// A wind schedule (rq_env_set_wind_schedule): the bank's tables and the env's per-env first rows (rq_device_math.hpp wind_*).
struct WindPtrs {
    const float* rows;        // [n_tables * n_rows][4] row-major: air velocity (world frame, m/s), specific drag (1/s); nullptr = none
    const uint32_t* row0;     // [ld]: wind_id[i] * n_rows, the first row of env i's table
    uint32_t n_rows;          // rows of one table
    uint32_t pad_;
};

// A delay schedule (rq_env_set_delay_schedule): the bank's tables, the env's per-env first rows and the env's command history
// (rq_device_math.hpp delay_*).  The history is a ring of kDelaySlots slots x 4 action fields x ld: the slot of the command given at
// episode step k is k mod kDelaySlots.  Twice the longest delay: the slot a step reads (k - d, 1 <= d <= RQ_DELAY_MAX_STEPS) is never
// the slot it writes (k).
constexpr uint32_t kDelaySlots = 2u * RQ_DELAY_MAX_STEPS;
static_assert((kDelaySlots & (kDelaySlots - 1u)) == 0, "the slot of a step is a mask of its count");
struct DelayPtrs {
    const uint8_t* rows;      // [n_tables * n_rows]: the delay in steps, 0 .. RQ_DELAY_MAX_STEPS; nullptr = none
    const uint32_t* row0;     // [ld]: delay_id[i] * n_rows, the first row of env i's table
    float* ring;              // [kDelaySlots][4][ld]: the commands the env's actor gave, by episode step
    uint32_t n_rows;          // rows of one table
    uint32_t pad_;
};

// A sensor schedule (rq_env_set_sensor_schedule): the bank's tables, the env's per-env first rows and the env's readings
// (rq_device_math.hpp sensor_*).  The readings are a ring of kSensorSlots slots x kSensorFields observation fields x ld: the slot of
// the reading assembled at episode step k is k mod kSensorSlots.  Twice the longest delay: the slot an observation reads (k - d',
// 1 <= d' <= RQ_SENSOR_MAX_STEPS) is never the slot it writes (k).
constexpr uint32_t kSensorSlots = 2u * RQ_SENSOR_MAX_STEPS;
constexpr uint32_t kSensorFields = 18;      // position, rotation matrix, linear and angular velocity: the observation's columns 0..17
static_assert((kSensorSlots & (kSensorSlots - 1u)) == 0, "the slot of a step is a mask of its count");
struct SensorPtrs {
    const uint8_t* rows;      // [n_tables * n_rows]: the delay in steps, 0 .. RQ_SENSOR_MAX_STEPS; nullptr = none
    const uint32_t* row0;     // [ld]: sensor_id[i] * n_rows, the first row of env i's table
    float* ring;              // [kSensorSlots][kSensorFields][ld]: the readings assembled for the env, by episode step
    uint32_t n_rows;          // rows of one table
    uint32_t pad_;
};

// SampleAndSquash output stage of the actor (rq_policy_set_sample_and_squash): mode = rq_sample_and_squash_mode
struct SasArgs {
    uint32_t mode;                // RQ_SAS_OFF / RQ_SAS_MEAN / RQ_SAS_SAMPLE
    uint32_t epoch;               // sampling counter of this launch (+ *epoch_base inside a replayed hipGraph)
    const uint32_t* epoch_base;
    const float* ls_image;        // 20 x 64 floats: log-std head operands + bias (pack_logstd_head), RQ_SAS_SAMPLE only
    uint64_t seed;
    uint64_t env_offset;          // global id of batch element 0 (k_actor_step; the fused kernel has its Batch)
};

struct Batch {           // which envs a launch covers
    uint32_t n, ld;      // envs, leading dimension of every SoA buffer
    uint64_t env_offset; // global id of env 0 (RNG key)
};

// Small-batch hand-over to/from the host without a copy command or a stream synchronisation: the kernel
// reads its input rows from / mirrors its output rows into pinned host memory and the last workgroup to
// finish publishes `seq` in a pinned flag the host spins on (measured: 7.3 us per launch + result against
// 14.3 us for kernel + hipMemcpyAsync + hipStreamSynchronize, tools/synclat.hip).  All-null = not used.
struct Mailbox {
    const float* rows_in;   // row-major input [n][in_stride] replacing the field-major one, or nullptr
    uint32_t in_stride;
    float* rows_out;        // row-major mirror [n][dim] of the kernel's output, or nullptr
    uint32_t* counter;      // device: workgroups finished (left at 0)
    uint32_t* flag;         // pinned host: receives seq when every workgroup is done, or nullptr
    uint32_t seq;
};
constexpr bool mailbox_used(const Mailbox& mb) { return mb.rows_in != nullptr || mb.rows_out != nullptr || mb.flag != nullptr; }

// ---- the actor step: Raptor.evaluate_step (README.md:97) ---------------------------------------------------------------------------
// obs [>= 22][ld_obs] -> act [4][ld_act]; hidden [16][ld_h] in / out.  Set the fields by name; what a launch does not use keeps
// its default.
struct ActorStepLaunch {
    uint32_t n = 0;                          // batch elements; 0: nothing to do
    // One policy: `packed` is its MFMA A-operand image in `precision` (rq::pack_policy[_bf16 | _f16x2]).  A policy bank (fp32; no host
    // rows, no output stage, no speculation): images [P][RQ_PACKED_FLOATS] and block_policy [ceil(n / 64)], the policy of each 64-env
    // block; policy_interval [P] (every entry 1 .. RQ_POLICY_MAX_NATIVE_INTERVAL) set: the bank's rate step, which needs `steps`.
    const float* packed = nullptr;
    const float* images = nullptr;
    const uint32_t* block_policy = nullptr;
    const uint32_t* policy_interval = nullptr;
    const float* obs = nullptr;  uint32_t ld_obs = 0;
    float* hidden = nullptr;                 // read and written ...
    const float* hidden_in = nullptr;        // ... unless set: the state BEFORE the step is read here, `hidden` only written (speculation)
    uint32_t ld_h = 0;
    float* act = nullptr;  uint32_t ld_act = 0;
    const uint8_t* frozen = nullptr;         // set: rows with frozen[i] != 0 are skipped (rollout semantics)
    int precision = RQ_POLICY_FP32;          // rq_policy_precision
    SasArgs sas{};                           // the optional SampleAndSquash output stage
    Mailbox mb{};                            // host rows in / out (below 1 024 envs)
    // The rate rule of one policy, interval > 1 (rq_policy_set_native_interval; a bank's intervals are its table's): the actions are
    // written as ever, the hidden state only for the rows at a native step - steps set: row i iff steps[i] % interval == 0 (the
    // chained rollout: the env's episode step count at observe time); steps null: every row iff native (evaluate_step: one call
    // counter for the batch).
    const uint32_t* steps = nullptr;
    uint32_t interval = 1;
    bool native = false;
};

enum class ActorFamily { UNSUPPORTED, STEP, STREAM, RATE, BANK, BANK_RATE };      // k_actor_step, _stream, _step_rate, _step_bank, _step_rate_bank
enum class ActorBuild { F32_LEAN, BF16, F16X2 };                                  // ActorF32Lean, ActorBF16, ActorF16X2

struct ActorStepTraits {
    uint32_t n;             // batch elements
    int precision;          // rq_policy_precision
    bool bank, rated;       // a policy bank acts; the rate rule applies (one policy: interval > 1; a bank: it has its interval table)
    bool mailbox;           // host rows or the host flag
    bool sas;               // a SampleAndSquash stage is on
    bool hidden_in;         // the state is read from a buffer of its own
    uint32_t ld_max;        // max(ld_h, ld_obs)
    uint32_t forced_gpw;    // RQ_ACTOR_GROUPS_PER_WAVE (launch-shape sweeps, tools/actor_gpw_sweep.py); 0: not set
};

struct ActorStepRoute { ActorFamily family; ActorBuild build; uint32_t groups_per_wave, grid; };      // grid: workgroups of kActorBlock

constexpr uint32_t kActorBlock = 256;      // rq_rollout.hpp kBlock: 4 waves

// 64-env groups one wave of the actor step works through at n envs (1 = k_actor_step); bench.py's actor_groups_per_wave mirrors
// this.  From 262 144 envs on the launch keeps ~1 024 waves - one per SIMD - and lets each stream through groups / 1 024 groups, so
// that the per-wave operand-image load (18 KB, more than a group's own 14.8 KB of data) is amortised (tools/actor_gpw_sweep.py,
// round 4: 1 048 576 envs 61.5 us with 16 groups per wave against 103 with 32 = 512 waves; 2 097 152 envs 119 - 124 us with 32
// against 128 with 8 and 137 with 1 or 16)
constexpr uint32_t actor_groups_per_wave(uint32_t n) {
    const uint32_t groups = (n + 63u) / 64u;
    if (groups < 4096u) return 1u;
    const uint32_t g = groups / 1024u;
    return g > 64u ? 64u : g;
}

constexpr ActorStepRoute route_actor_step(const ActorStepTraits& t) {
    const bool bf16 = t.precision == RQ_POLICY_BF16_MFMA, f16x2 = t.precision == RQ_POLICY_F16X2_MFMA;
    // the fp32 build is the two-tiles-per-pass one in every family (~30 registers fewer live, 2-3 % faster at every size): one
    // policy's and a bank's steps are the same bits
    const ActorBuild build = f16x2 ? ActorBuild::F16X2 : bf16 ? ActorBuild::BF16 : ActorBuild::F32_LEAN;
    // What no kernel is built for: a bank in 16 bits, with host rows or an output stage; a rate step that speculates or has that stage.
    if ((t.bank && (bf16 || f16x2 || t.mailbox || t.sas || t.hidden_in)) || (t.rated && (t.hidden_in || t.sas)))
        return {ActorFamily::UNSUPPORTED, build, 0, 0};
    const uint32_t groups = (t.n + 63u) / 64u;
    const uint32_t per_block = kActorBlock / 64u;
    // a bank's kernels and the rate kernel: one 64-env group per wave at every batch size
    if (t.bank) return {t.rated ? ActorFamily::BANK_RATE : ActorFamily::BANK, build, 1, (groups + per_block - 1) / per_block};
    if (t.rated) return {ActorFamily::RATE, build, 1, (groups + per_block - 1) / per_block};
    // The streaming kernel: several groups per wave, no host rows (they exist below 1 024 envs only) and every byte offset of its
    // buffer instructions in 31 bits (26 field rows of 4 ld bytes); otherwise one group per wave.
    const uint32_t gpw = t.forced_gpw ? t.forced_gpw : actor_groups_per_wave(t.n);
    const bool stream = gpw > 1 && !t.mailbox && (uint64_t)t.ld_max * 4u * 26u < 0x7FFFFFFFull;
    if (!stream) return {ActorFamily::STEP, build, 1, (groups + per_block - 1) / per_block};
    const uint32_t waves = (groups + gpw - 1) / gpw;
    return {ActorFamily::STREAM, build, gpw, (waves + per_block - 1) / per_block};
}

constexpr ActorStepTraits actor_step_traits(const ActorStepLaunch& a, uint32_t forced_gpw) {
    return {a.n, a.precision, a.block_policy != nullptr, a.block_policy != nullptr ? a.policy_interval != nullptr : a.interval > 1,
            mailbox_used(a.mb), a.sas.mode != RQ_SAS_OFF, a.hidden_in != nullptr, a.ld_h > a.ld_obs ? a.ld_h : a.ld_obs, forced_gpw};
}

// ---- the env step: vector.step (README.md:98) + reward / termination / statistics ----------------------------------------------------
struct EnvStepLaunch {
    Batch b{}; StepCfg c{};
    const float* params = nullptr;
    const float* state = nullptr;            // read ...
    float* action = nullptr;                 // [4][ld]; with mb.rows_in the actions come from the mailbox and are also written here
    float* next_state = nullptr;             // ... written (a rollout steps in place: next_state == state)
    StatsPtrs st{};
    bool rollout = false;                    // the episode-end handling of rq_rollout: freeze, or under RQ_ROLLOUT_AUTORESET in `flags`
    uint32_t flags = 0;                      // re-sample (sc, seed) and reset the policy state:
    SampleCfg sc{}; uint64_t seed = 0;
    float* hidden = nullptr;                 // [16][ld] <- the initial state in `weights` (checkpoint order), or, block_policy
    const float* weights = nullptr;          // [ceil(n / 64)] set, in block block_policy[i >> 6] of weights [P][RQ_POLICY_NUM_WEIGHTS]
    const uint32_t* block_policy = nullptr;  // (a bank's step: a rollout's, in place, without host rows or a folded observation)
    Mailbox mb{};
    // set: the observation of the state just written (after an auto-reset: of the re-sampled one), as vector.observe would assemble
    // it - with the noise draw of epoch obs_epoch + *obs_epoch_base when `noise` - goes to obs_of_next [RQ_OBSERVATION_DIM][ld] and,
    // row-major, to mb.rows_out
    float* obs_of_next = nullptr;
    NoiseCfg nc{}; bool noise = false; uint32_t obs_epoch = 0; const uint32_t* obs_epoch_base = nullptr;
    WrenchPtrs wr{};                         // rows set: the env's wrench schedule
    VehiclePtrs vh{};                        // rows set: the env's vehicle schedule (not used: the kernels without it)
    WindPtrs wd{};                           // rows set: the env's wind schedule (not used: the kernels without it)
    DelayPtrs dl{};                          // rows set: the env's delay schedule (not used: the kernels without it)
    SensorPtrs sn{};                         // rows set: the env's sensor schedule; no step kernel reads it (k_sensor_apply delivers
                                             // behind the step that folds the next observation: launch_sensor_apply)
    // The thaw of a chained rollout under auto-reset reads b, sc, seed, params, st, hidden, weights and block_policy, and re-samples
    // into next_state.
};

// Which kernel serves an env step (launch_step switches on the answer).  The kernels are built nested, each family taking the
// schedules inside it as template bools: delay > wind > vehicle > wrench > none - k_step<rollout>, k_step_wrench<rollout>,
// k_step_vehicle<rollout, wrench>, k_step_wind<rollout, wrench, vehicle>, k_step_delay<rollout, wrench, vehicle, wind> and, for a bank,
// k_step_bank, k_step_bank_wrench, k_step_bank_vehicle<wrench>, k_step_bank_wind<wrench, vehicle>, k_step_bank_delay<wrench, vehicle,
// wind>.  `family` is the outermost schedule attached.  A bank's step is a rollout's, in place, without host rows or a folded
// observation.  A sensor schedule (e.sn) changes nothing here: the step is the step it would be without it.
enum class EnvStepFamily { NONE, WRENCH, VEHICLE, WIND, DELAY };      // the nesting order, innermost first
struct EnvStepRoute {
    bool supported, bank, rollout;
    bool wrench, vehicle, wind, delay;      // which schedules are attached
    EnvStepFamily family;
};
inline EnvStepRoute route_env_step(const EnvStepLaunch& e) {
    const bool bank = e.block_policy != nullptr;
    const bool supported = !bank || (e.rollout && e.next_state == e.state && !mailbox_used(e.mb) && e.obs_of_next == nullptr);
    const bool wrench = e.wr.rows != nullptr, vehicle = e.vh.rows != nullptr, wind = e.wd.rows != nullptr, delay = e.dl.rows != nullptr;
    const EnvStepFamily family = delay ? EnvStepFamily::DELAY
                                 : wind ? EnvStepFamily::WIND
                                 : vehicle ? EnvStepFamily::VEHICLE
                                 : wrench ? EnvStepFamily::WRENCH
                                          : EnvStepFamily::NONE;
    return {supported, bank, e.rollout, wrench, vehicle, wind, delay, family};
}

}  // namespace rq
