/*
 * raptor_quad.h — C ABI of the MI355X-native vectorised quadrotor rollout engine.
 *
 * This is the drop-in boundary for the rollout hot path of rl-tools/raptor.  Every entry
 * point replaces one call site of the reference's Python/C++ surface (citations are
 * /root/reference/README.md:<line>; "checkpoint.h:<line>" is the generated policy export
 * inside data/raptor-policy-checkpoint.tar.gz):
 *
 *   reference call (README.md)                                   this ABI
 *   -----------------------------------------------------------  ---------------------------------
 *   l2f.Device()                                        :49      rq_device_create
 *   vector.VectorRng()                                  :50      rq_rng_create
 *   vector.VectorEnvironment()  (.N_ENVIRONMENTS,
 *                                .OBSERVATION_DIM)      :51,55   rq_env_create / rq_env_num_envs / RQ_OBSERVATION_DIM
 *   vector.VectorParameters()                           :53      rq_params_create
 *   vector.VectorState()   (.states[i].position,
 *                           .assign(), copy)            :54,56,73-75,99   rq_state_create / rq_state_assign / rq_state_{get,set}
 *   vector.initialize_rng(device, rng, seed)            :58      rq_initialize_rng
 *   vector.initialize_environment(device, env)          :59      rq_initialize_environment
 *   vector.sample_initial_parameters(device, env,
 *                                    params, rng)       :60      rq_sample_initial_parameters
 *   vector.sample_initial_state(device, env, params,
 *                               state, rng)             :61      rq_sample_initial_state
 *   vector.observe(device, env, params, state,
 *                  observation, rng)                    :96      rq_observe
 *   vector.step(device, env, params, state, action,
 *               next_state, rng) -> dts                 :98      rq_step
 *   foundation_policy.Raptor()                          :20,48   rq_policy_create (+ rq_policy_set_weights)
 *   Raptor.reset()                                      :21,94   rq_policy_reset
 *   Raptor.evaluate_step(obs[B,22]) -> act[B,4]         :24,97   rq_policy_evaluate_step
 *   the loop body README.md:95-99 x K                            rq_rollout  (fused or hipGraph-chained)
 *   boot self-test of the embedded backend              :136-139,155   rq_policy_selftest
 *   rl_tools_inference_applications_l2f_control(...)->status :163      convention: POD in/out, int status
 *   rl-tools layers standardize / sample_and_squash     :114,116 rq_policy_set_standardize / rq_policy_set_sample_and_squash
 *   post-training data collection                       :208     rq_rollout_record + rq_trajectory_*
 *   distillation: ~1000 MLP teachers queried on
 *     student-visited states                            :208-216 rq_teacher_bank_create / rq_trajectory_relabel_teachers
 *   distillation: the teachers flying their own
 *     quadrotors (checks, teacher-acting collection)    :207-216 rq_rollout_teachers / rq_teacher_bank_evaluate
 *     ... on a moving setpoint, one table or one per env          rq_rollout_teachers_track / rq_rollout_teachers_track_refs
 *   distillation: the student's regression gradient    :208-216 rq_trajectory_policy_forward / _backward + rq_policy_set_weights;
 *                                                              rq_trajectory_distill (loss, Adam and repack on the device);
 *                                                              rq_trajectory_*_weighted (a weight per env or per env and step)
 *   distillation: which teachers the student imitates
 *     badly, and how the error falls with episode age   :208-216 rq_trajectory_policy_error_table / rq_trajectory_policies_error_table
 *   (the reference is single-process) env shards over
 *     GPUs + all-gather of episode returns (RCCL)                rq_env_create(global_env_offset) / rq_comm_* / rq_allgather_returns
 *
 * The entry points under "DIAGNOSTICS" at the end of this header (timers, per-wave records, launch floor, speculation knobs)
 * replace nothing of the reference: they are this engine's own instrumentation and stand outside the drop-in table.
 *
 * Conventions
 *   - Every function returns an int status: RQ_OK (0) or a negative rq_status; the message of
 *     the last failure on the calling thread is available from rq_last_error().  Nothing
 *     throws across the boundary.
 *   - Host buffers are caller-owned, C-contiguous float32, row-major [n_envs, dim] exactly as
 *     the reference's NumPy arrays (README.md:55,92).  Passing NULL for an observation /
 *     action pointer means "use the device-resident buffer of the env / policy" (no PCIe
 *     traffic): the chain observe(NULL) -> evaluate_step(NULL,NULL) -> step(NULL) never
 *     leaves HBM.
 *   - One rq_device = one HIP device + one HIP stream.  Calls on objects of one rq_device are
 *     not re-entrant; objects of different rq_devices are independent.  Calls that return
 *     host data are synchronous w.r.t. that data; everything else is asynchronous on the
 *     device stream (rq_device_synchronize waits).  Host input arrays are pageable memory and are
 *     fully read before the call returns (the caller may reuse them at once).
 *   - Batch size is a runtime value (the reference bakes it into the module name "vector8").
 *   - Device data is struct-of-arrays, field-major: field f of env i lives at base[f*ld + i]
 *     (ld = n_envs rounded up to 64), so a wavefront's 64 lanes read 256 contiguous bytes.
 */
#ifndef RAPTOR_QUAD_H
#define RAPTOR_QUAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RQ_ABI_VERSION 5   /* 2 (round 3): rq_env_config.action_history_raw; termination_position default 1 m; the entry points added in
                              rounds 2 and 3 (the latter: rq_device_last_rollout_waves)
                              3 (round 4): rq_device_{set,get}_speculation, rq_device_last_rollout_clock; no struct changed
                              4 (round 5): rq_comm_describe (new struct rq_comm_description); rq_comm_info / rq_comm_create ask RCCL for
                              the communicator's own rank and size; rq_teacher_bank_create_layers
                              5 (round 6): rq_device_{set,get}_resident; no struct changed
                              (still 5: rq_policy_{set,get}_native_interval added, no struct changed)
                              (still 5: rq_policy_bank_* and rq_rollout_policies, then rq_bank_optimizer_* and rq_trajectory_policies_*
                              added, no struct changed)
                              (still 5: rq_policy_bank_{set,get}_native_interval and rq_rollout_policies_track added, no struct changed)
                              (still 5: rq_reference_bank_{create,destroy}, rq_rollout_track_refs and rq_rollout_policies_track_refs added,
                              no struct changed)
                              (still 5: rq_rollout_teachers_track and rq_rollout_teachers_track_refs added, no struct changed)
                              (still 5: rq_wrench_bank_{create,destroy} and rq_env_{set,get}_wrench_schedule added, no struct changed)
                              (still 5: rq_vehicle_bank_{create,destroy} and rq_env_{set,get}_vehicle_schedule added, no struct changed)
                              (still 5: rq_wind_bank_{create,destroy} and rq_env_{set,get}_wind_schedule added, no struct changed)
                              (still 5: rq_delay_bank_{create,destroy} and rq_env_{set,clear,get}_delay_schedule added, no struct changed)
                              (still 5: rq_sensor_bank_{create,destroy} and rq_env_{set,clear,get}_sensor_schedule added, no struct changed)
                              (still 5: rq_optimizer_{get,set}_state, rq_optimizer_apply and rq_bank_optimizer_{get,set}_state added, no
                              struct changed) */

#if defined(__GNUC__)
#define RQ_API __attribute__((visibility("default")))
#else
#define RQ_API
#endif

/* ---- sizes fixed by the checkpoint / observation spec ---------------------------------- */
#define RQ_POLICY_INPUT_DIM 22   /* checkpoint.h:62  Shape<500,2,22>; README.md:23            */
#define RQ_POLICY_HIDDEN_DIM 16  /* checkpoint.h:134 gru::Configuration<float,...,16,...>      */
#define RQ_POLICY_OUTPUT_DIM 4   /* checkpoint.h:170,211                                        */
#define RQ_POLICY_NUM_WEIGHTS 2084 /* W0[16,22] b0[16] Wi[48,16] Wh[48,16] bi[48] bh[48] h0[16] W2[4,16] b2[4] */
#define RQ_ACTION_DIM 4          /* motor commands FR,BR,BL,FL in [-1,1]  (README.md:27)        */
/* observation = policy-visible head (22) + privileged tail (4 normalised rotor speeds);
 * the caller slices [:, :22] exactly as README.md:97 does. */
#define RQ_OBSERVATION_DIM 26

/* ---- per-env parameter fields (float32 each), SoA field index -------------------------- */
enum rq_param_field {
    RQ_P_MASS = 0,
    RQ_P_JXX = 1, RQ_P_JYY = 2, RQ_P_JZZ = 3,   /* diagonal inertia, body frame [kg m^2]        */
    RQ_P_ROTOR_POS = 4,                          /* 4 rotors x (x,y,z) body frame [m], 12 fields */
    RQ_P_THRUST_C0 = 16, RQ_P_THRUST_C1 = 17, RQ_P_THRUST_C2 = 18, /* T = c0 + c1 r + c2 r^2 [N] */
    RQ_P_TORQUE_CONST = 19,                      /* yaw reaction torque per unit thrust [m]      */
    RQ_P_TAU_RISE = 20, RQ_P_TAU_FALL = 21,      /* first-order rotor time constants [s]         */
    RQ_P_RPM_MIN = 22, RQ_P_RPM_MAX = 23,        /* action -1 / +1 map to these rotor speeds     */
    RQ_P_HOVER_RPM = 24,                         /* rotor speed at which 4 T = m g               */
    RQ_P_HOVER_ACTION = 25,                      /* the same, in normalised action units         */
    RQ_PARAM_DIM = 26
};

/* ---- per-env state fields (float32 each), SoA field index ------------------------------ */
enum rq_state_field {
    RQ_S_POS = 0,        /* 3: position, world frame FLU [m]                                     */
    RQ_S_QUAT = 3,       /* 4: orientation quaternion (w,x,y,z), body -> world                  */
    RQ_S_VEL = 7,        /* 3: linear velocity, world frame [m/s]                                */
    RQ_S_OMEGA = 10,     /* 3: angular velocity, body frame [rad/s]                              */
    RQ_S_RPM = 13,       /* 4: rotor speeds                                                      */
    RQ_S_LAST_ACTION = 17, /* 4: previous action = ActionHistory(1): clipped, or raw (action_history_raw) */
    RQ_S_FORCE = 21,     /* 3: per-episode disturbance force, world frame [N]                    */
    RQ_S_TORQUE = 24,    /* 3: per-episode disturbance torque, body frame [N m]                  */
    RQ_STATE_DIM = 27
};

typedef enum rq_status {
    RQ_OK = 0,
    RQ_ERR_INVALID_ARGUMENT = -1,
    RQ_ERR_NO_DEVICE = -2,        /* no HIP device / HIP runtime failure at creation            */
    RQ_ERR_HIP = -3,              /* a HIP call failed (message in rq_last_error)               */
    RQ_ERR_OUT_OF_MEMORY = -4,
    RQ_ERR_SHAPE_MISMATCH = -5,   /* objects belong to different envs / devices / batch sizes   */
    RQ_ERR_NOT_INITIALIZED = -6,  /* e.g. observe before initialize_environment                 */
    RQ_ERR_SELFTEST_FAILED = -7
} rq_status;

/* Static MDP configuration shared by all envs of a VectorEnvironment
 * (what vector.initialize_environment fills, README.md:59).  Plain data; copied on set. */
typedef struct rq_env_config {
    uint32_t struct_size;               /* = sizeof(rq_env_config), checked on set              */
    /* integration */
    float dt;                           /* 0.01 s: "simulation dt=10 ms" README.md:25           */
    float gravity;                      /* 9.81, acts along world -z                            */
    uint32_t episode_step_limit;        /* 500: README.md:95, checkpoint.h:62                   */
    /* per-env parameter sampling */
    uint32_t domain_randomization;      /* 0: nominal Crazyflie for every env; 1: scaling law   */
    float dr_scale_min, dr_scale_max;               /* length scale s ~ U[.,.] (0.5, 8)          */
    float dr_thrust_to_weight_min, dr_thrust_to_weight_max; /* (1.5, 5)                          */
    float dr_torque_const_min, dr_torque_const_max;         /* x s  (0.005, 0.03)                */
    float dr_motor_tau_min, dr_motor_tau_max;               /* (0.03, 0.2) s                     */
    /* initial-state sampling */
    float init_guidance;                /* probability of the hover-at-origin state (0.1)       */
    float init_max_position;            /* 0.5 m, per axis                                      */
    float init_max_angle;               /* pi/2 rad about a uniform random axis                 */
    float init_max_linear_velocity;     /* 1 m/s per axis                                       */
    float init_max_angular_velocity;    /* 1 rad/s per axis                                     */
    /* per-episode constant disturbances, std relative to m g (force) and m g * arm (torque)  */
    float disturbance_force_std;        /* 0 = off                                              */
    float disturbance_torque_std;       /* 0 = off                                              */
    /* observation noise (std); all zero = no RNG draw */
    float noise_position, noise_orientation, noise_linear_velocity, noise_angular_velocity;
    /* reward = terminated ? termination_penalty : constant - scale * weighted cost */
    float reward_scale, reward_constant, reward_termination_penalty;
    float reward_position, reward_orientation, reward_linear_velocity,
          reward_angular_velocity, reward_action;
    /* termination: |p_i| > .. (default 1 m [UPSTREAM-UNVERIFIED]: fitted - the value at which the shipped policy reproduces
     * the sampled-quadrotor share_terminated / episode_length of the reference's own training log; its nominal-Crazyflie
     * record is NOT reproduced), |v_i| > .., |w_i| > .. (any axis)
     * or any non-finite state */
    uint32_t termination_enabled;
    float termination_position, termination_linear_velocity, termination_angular_velocity;
    /* ActionHistory(1) of the observation (h5:/actor@meta): 0 = the action as the rotors received it, clipped to
     * [-1, 1] (default); 1 = the policy's raw output.  Which one l2f stores is not in the reference tree
     * [UPSTREAM-UNVERIFIED]; the shipped actor's output is unbounded (checkpoint.h:210 reaches +-3), so the two
     * differ on saturated steps (measured effect on the closed-loop statistics: DESIGN.md section 2). */
    uint32_t action_history_raw;
} rq_env_config;

typedef struct rq_device rq_device;   /* l2f.Device                                             */
typedef struct rq_rng rq_rng;         /* vector.VectorRng                                       */
typedef struct rq_env rq_env;         /* vector.VectorEnvironment                               */
typedef struct rq_params rq_params;   /* vector.VectorParameters                                */
typedef struct rq_state rq_state;     /* vector.VectorState                                     */
typedef struct rq_policy rq_policy;   /* foundation_policy.Raptor                               */

/* ---- library ---------------------------------------------------------------------------- */
RQ_API int rq_abi_version(void);
RQ_API const char* rq_last_error(void);
RQ_API const char* rq_status_string(int status);
RQ_API int rq_device_count(int* count);

/* ---- Device (README.md:49) ------------------------------------------------------------- */
RQ_API int rq_device_create(int hip_device_ordinal, rq_device** out);
RQ_API int rq_device_destroy(rq_device* dev);
RQ_API int rq_device_synchronize(rq_device* dev);
/* raw hipStream_t of the device, for callers that enqueue their own work behind ours */
RQ_API int rq_device_stream(rq_device* dev, void** hip_stream);

/* ---- Rng (README.md:50,58) -------------------------------------------------------------
 * Counter-based Philox4x32-10: key = seed, counter = (block, epoch|episode, GLOBAL env id,
 * purpose).  Results depend only on (seed, global env id, call history), never on how envs
 * are sharded over devices. */
RQ_API int rq_rng_create(rq_device* dev, rq_rng** out);
RQ_API int rq_rng_destroy(rq_rng* rng);
RQ_API int rq_initialize_rng(rq_device* dev, rq_rng* rng, uint64_t seed);
RQ_API int rq_rng_get(const rq_rng* rng, uint64_t* seed, uint32_t* epoch);
RQ_API int rq_rng_set_epoch(rq_rng* rng, uint32_t epoch);

/* ---- Environment (README.md:51,59) ----------------------------------------------------- */
/* n_envs envs whose global ids are [global_env_offset, global_env_offset + n_envs). */
RQ_API int rq_env_create(rq_device* dev, uint32_t n_envs, uint64_t global_env_offset, rq_env** out);
RQ_API int rq_env_destroy(rq_env* env);
RQ_API int rq_env_num_envs(const rq_env* env, uint32_t* n_envs);
RQ_API int rq_env_leading_dim(const rq_env* env, uint32_t* ld);
RQ_API int rq_env_default_config(rq_env_config* cfg);                 /* fills the documented defaults */
RQ_API int rq_initialize_environment(rq_device* dev, rq_env* env);    /* = set default config          */
RQ_API int rq_env_set_config(rq_env* env, const rq_env_config* cfg);
RQ_API int rq_env_get_config(const rq_env* env, rq_env_config* cfg);

/* ---- Parameters / State containers (README.md:53,54,56,99) ---------------------------- */
RQ_API int rq_params_create(rq_env* env, rq_params** out);
RQ_API int rq_params_destroy(rq_params* p);
/* host copies are row-major [n_envs, RQ_PARAM_DIM] */
RQ_API int rq_params_get(const rq_params* p, float* host_out);
RQ_API int rq_params_set(rq_params* p, const float* host_in);
RQ_API int rq_params_device_ptr(const rq_params* p, float** dev_ptr); /* SoA base, ld = env ld        */

RQ_API int rq_state_create(rq_env* env, rq_state** out);
RQ_API int rq_state_destroy(rq_state* s);
RQ_API int rq_state_assign(rq_state* dst, const rq_state* src);       /* state.assign(next_state)      */
RQ_API int rq_state_get(const rq_state* s, float* host_out);          /* [n_envs, RQ_STATE_DIM]        */
RQ_API int rq_state_set(rq_state* s, const float* host_in);
RQ_API int rq_state_device_ptr(const rq_state* s, float** dev_ptr);

/* ---- the five l2f vector:: functions (README.md:60,61,96,98) --------------------------- */
RQ_API int rq_sample_initial_parameters(rq_device* dev, rq_env* env, rq_params* params, rq_rng* rng);
RQ_API int rq_sample_initial_state(rq_device* dev, rq_env* env, const rq_params* params,
                            rq_state* state, rq_rng* rng);
/* observation: host [n_envs, RQ_OBSERVATION_DIM] or NULL (stay in the env's device buffer) */
RQ_API int rq_observe(rq_device* dev, rq_env* env, const rq_params* params, const rq_state* state,
               float* observation, rq_rng* rng);
/* action: host [n_envs, RQ_ACTION_DIM] or NULL (= the env's device action buffer, which
 * rq_policy_evaluate_step(obs=NULL, act=NULL) fills).  dts: host [n_envs] or NULL.
 * Also evaluates reward and termination of the transition into the env's episode
 * statistics (see rq_env_get_*). state and next_state may be the same object. */
RQ_API int rq_step(rq_device* dev, rq_env* env, const rq_params* params, const rq_state* state,
            const float* action, rq_state* next_state, rq_rng* rng, float* dts);

/* device-resident observation [RQ_OBSERVATION_DIM][ld] and action [RQ_ACTION_DIM][ld] */
RQ_API int rq_env_observation_device_ptr(const rq_env* env, float** dev_ptr);
RQ_API int rq_env_action_device_ptr(const rq_env* env, float** dev_ptr);
RQ_API int rq_env_get_observation(const rq_env* env, float* host_out); /* [n_envs, RQ_OBSERVATION_DIM] */
RQ_API int rq_env_get_action(const rq_env* env, float* host_out);      /* [n_envs, RQ_ACTION_DIM]      */
RQ_API int rq_env_set_action(rq_env* env, const float* host_in);

/* ---- episode statistics (reward / termination of transitions taken by rq_step/rq_rollout) */
/* dst_is_device: 0 = host pointer; 1 = device pointer on the same HIP device (e.g. a torch tensor's
 * data_ptr()), copied on the env's stream and synchronised before return; 2 = device pointer, copy only
 * ENQUEUED on the env's stream (RQ_DST_DEVICE_ASYNC): order consumers behind rq_device_stream(), e.g. with an
 * event - this is how a collective overlaps the next rollout (bench.py). */
#define RQ_DST_HOST 0
#define RQ_DST_DEVICE 1
#define RQ_DST_DEVICE_ASYNC 2
RQ_API int rq_env_get_rewards(const rq_env* env, float* dst, int dst_is_device);          /* last transition */
RQ_API int rq_env_get_terminated(const rq_env* env, uint8_t* dst, int dst_is_device);     /* last transition */
RQ_API int rq_env_get_done_codes(const rq_env* env, uint8_t* dst, int dst_is_device);     /* last transition: 0 running, 1 terminated, 2 step limit, 4 frozen (not stepped) */
RQ_API int rq_env_get_frozen(const rq_env* env, uint8_t* dst, int dst_is_device);         /* 1: episode over, waits for sample_initial_state (rq_rollout without AUTORESET) */
RQ_API int rq_env_get_episode_index(const rq_env* env, uint32_t* dst, int dst_is_device); /* episodes started so far (RNG counter of the next reset) */
RQ_API int rq_env_get_returns(const rq_env* env, float* dst, int dst_is_device);          /* running episode */
RQ_API int rq_env_get_episode_steps(const rq_env* env, uint32_t* dst, int dst_is_device);
RQ_API int rq_env_get_finished_returns(const rq_env* env, float* dst, int dst_is_device); /* last finished episode */
RQ_API int rq_env_get_finished_lengths(const rq_env* env, uint32_t* dst, int dst_is_device);
RQ_API int rq_env_get_finished_counts(const rq_env* env, uint32_t* dst, int dst_is_device); /* #episodes finished */
RQ_API int rq_env_get_finished_terminated(const rq_env* env, uint32_t* dst, int dst_is_device); /* #of those that terminated */
/* Forget the episode bookkeeping: running and finished returns / lengths / counts, last reward, terminated and
 * done codes are zeroed AND the frozen flags are cleared - every env then counts as running a fresh episode
 * from whatever state it is in (what a caller that overwrites states with rq_state_set wants).  An env whose
 * episode had ended is NOT re-sampled by this call (rq_sample_initial_state does that, and also zeroes the
 * env's running return and step count).  The per-env episode counters that key the initial-state RNG are kept. */
RQ_API int rq_env_reset_statistics(rq_env* env);

/* ---- Policy (README.md:19-24,48,94,97; checkpoint.h:34-194) ---------------------------- */
typedef enum rq_policy_precision {
    RQ_POLICY_FP32 = 0,       /* exact fp32 on v_mfma_f32_16x16x4_f32 (one rounded fma per product), operands register-stationary */
    RQ_POLICY_BF16_MFMA = 1,  /* bf16 operands on v_mfma_f32_16x16x32_bf16, fp32 accumulate and gates */
    RQ_POLICY_F16X2_MFMA = 2  /* every operand as two f16 pieces (hi + lo, 22 significand bits or 2^-25 absolute) on
                                 v_mfma_f32_16x16x32_f16, exact products, fp32 accumulate and gates: known-answer error
                                 ~1e-6 like fp32, on the matrix pipe that overlaps with the vector ALU.  Not fp32
                                 arithmetic: RQ_POLICY_FP32 stays the default and the benchmarked configuration.
                                 Range (round 3): observations and layer_0's output are SATURATED at the largest f16,
                                 +-65 504 (a NaN input reads as -65 504), before they are split - an input beyond that is a
                                 bounded error (the gates saturate), never an infinity or NaN in the GRU state.
                                 WEIGHTS have no such clamp: an operand of magnitude >= 65 520 would split into hi = inf,
                                 lo = -inf, a NaN in every contraction it enters.  The operands are W0, b0, W2 as they are and
                                 the rows of Wi / Wh after their pre-scale (r and z rows x -log2 e, n rows x -2 log2 e: a
                                 weight of 22 708 in an n row is already out of range).  Such parameters are REFUSED with
                                 RQ_ERR_INVALID_ARGUMENT and a message that names the first offending weight index
                                 ("weight 1779 is outside the f16 range ..."): by rq_policy_set_precision(F16X2), by
                                 rq_policy_set_weights and rq_policy_set_standardize on a policy that is in F16X2 (the
                                 folded layer_0 counts), and by rq_policy_pack_image(F16X2).  The refused call changes
                                 nothing: precision, parameters, stages and every result stay what they were.  fp32 and
                                 bf16 carry such weights.  rq_teacher_bank_set_precision refuses likewise. */
} rq_policy_precision;

/* weights: RQ_POLICY_NUM_WEIGHTS float32 in the order documented at RQ_POLICY_NUM_WEIGHTS
 * (the order of checkpoint.h:39,50,75,87,99,111,123,149,160). */
RQ_API int rq_policy_create(rq_device* dev, const float* weights, size_t n_weights, rq_policy** out);
RQ_API int rq_policy_destroy(rq_policy* pol);
RQ_API int rq_policy_set_precision(rq_policy* pol, int precision);
/* Host only (no GPU involved): the per-lane register image the actor kernels of `precision` keep their operands in,
 * `*floats` = its size in 4-byte words (64 lanes x registers; layout: raptor_amd/csrc/rq_kernels.hpp QW_ / BW_ / FW_;
 * the f32 image is stored in quads of registers, rq::qw_slot, so that a lane fetches four with one 16-byte load).
 * `image` may be NULL to query the size.  A diagnostic: it lets the packing (pre-scaled gate rows, bf16 rounding,
 * the f16 hi / lo split) be checked without a device. */
RQ_API int rq_policy_pack_image(const float* weights, size_t n_weights, int precision, float* image, size_t capacity,
                                size_t* floats);
/* Optional stages named by rl-tools' layer list (README.md:114,116) that the SHIPPED checkpoint does not
 * contain (checkpoint.h:185 chains layer_0, layer_1, layer_2 only) — identity unless enabled; their
 * reference semantics are unpinned (no source or test vector in the reference tree):
 *   Standardize: x <- (x - mean) / std on the 22 inputs (folded into layer_0's weights, zero run-time cost);
 *                mean = std = NULL disables.
 *   Squash:      action <- tanh(action): SampleAndSquash in evaluation mode; the full layer (mean / log-std split,
 *                sampling) is rq_policy_set_sample_and_squash below. */
RQ_API int rq_policy_set_standardize(rq_policy* pol, const float* mean, const float* std);
RQ_API int rq_policy_set_squash(rq_policy* pol, int enable);   /* = set_sample_and_squash(RQ_SAS_MEAN / RQ_SAS_OFF) */
/* SampleAndSquash as a layer (rl-tools nn/layers/sample_and_squash [UPSTREAM-UNVERIFIED]): the last dense layer
 * has 8 outputs, [mean (4) | log_std (4)].  The 4 mean rows are the policy's layer_2; the 4 log-std rows are given
 * here: log_std_weights [4][16] row-major (NULL = state-independent log-std) and log_std_bias [4] (NULL = 0).
 *   RQ_SAS_OFF    raw output (the shipped checkpoint, checkpoint.h:170 IDENTITY)
 *   RQ_SAS_MEAN   action = tanh(mean)                                       (evaluation mode)
 *   RQ_SAS_SAMPLE action = tanh(mean + exp(clamp(log_std, -20, 2)) * eps), eps ~ N(0,1) drawn from Philox4x32-10
 *                 keyed by `seed`, counter (step, GLOBAL env id): rollouts use the rng's epoch as the step (fused
 *                 and chained modes agree bit for bit), rq_policy_evaluate_step a per-policy call counter that
 *                 rq_policy_reset rewinds.  Sequence evaluation and relabelling are deterministic passes and
 *                 reject this mode. */
typedef enum rq_sample_and_squash_mode { RQ_SAS_OFF = 0, RQ_SAS_MEAN = 1, RQ_SAS_SAMPLE = 2 } rq_sample_and_squash_mode;
RQ_API int rq_policy_set_sample_and_squash(rq_policy* pol, int mode, const float* log_std_weights,
                                    const float* log_std_bias, uint64_t seed);
/* The native interval R of a policy flown faster than it was trained (the reference's deployment section: a 2.5 ms control
 * interval against the 10 ms native one, "the native state progression in the policy is only triggered every 4 steps").
 * R = 1 .. RQ_POLICY_MAX_NATIVE_INTERVAL; 1 is the default and every call then does what it did before this entry point existed.
 * This engine's definition [UPSTREAM-UNVERIFIED] (which phase upstream's executor calls native, and whether its tentative
 * step starts before or after the last commit, are not in the reference tree):
 *   the call with index k computes (a, h') = step(o, h) with the arithmetic of R = 1 and returns a;
 *   h <- h' iff k % R == 0 (a native step); otherwise h stays, and the next call is again a tentative step from the last
 *   committed state.
 * k is, in rollouts (rq_rollout, rq_rollout_record, rq_rollout_track, both modes), the env's own episode step count at observe
 * time - the count a tracked rollout indexes its table with: the first step of every episode is native, an env that auto-resets
 * gets the initial hidden state and k = 0, a frozen env changes nothing, and the phase crosses launches in the env's step count;
 * in rq_policy_evaluate_step, a per-policy call counter, one for the whole batch, that rq_policy_reset and this call rewind.
 * The env side is untouched: the previous action in the observation stays the action last applied.
 * Setting R keeps weights, precision and hidden state.  Refused, with rq_last_error naming the interval and nothing changed:
 * R = 0 or above the maximum; R > 1 beside a SampleAndSquash stage (whichever is set second); and with R > 1
 * rq_policy_evaluate_sequence, rq_policy_selftest, rq_trajectory_relabel, rq_trajectory_policy_forward / _backward /
 * _loss_grad and rq_trajectory_distill - a recording does not carry the phase it started at, and training is at the native
 * rate.  The small-batch loop neither speculates nor keeps a resident executor for such a policy: its calls are plain launches. */
#define RQ_POLICY_MAX_NATIVE_INTERVAL 64
RQ_API int rq_policy_set_native_interval(rq_policy* pol, uint32_t interval);
RQ_API int rq_policy_get_native_interval(const rq_policy* pol, uint32_t* interval);
/* hidden state h[B,16] <- initial_hidden_state (checkpoint.h:123); sized on first use */
RQ_API int rq_policy_reset(rq_policy* pol);
/* One recurrent step for a batch.  observation: host [batch, obs_stride] (first 22 columns
 * used, obs_stride >= 22) -> action host [batch, 4]; output is the raw Dense output (not
 * squashed/clipped, checkpoint.h:170 IDENTITY).  With env != NULL and observation == NULL the
 * env's device observation buffer is read; with action == NULL the env's device action
 * buffer is written. batch must stay constant between resets. */
RQ_API int rq_policy_evaluate_step(rq_policy* pol, rq_env* env, const float* observation,
                            uint32_t batch, uint32_t obs_stride, float* action);
RQ_API int rq_policy_get_hidden(const rq_policy* pol, float* host_out, uint32_t batch); /* [batch,16] */
RQ_API int rq_policy_set_hidden(rq_policy* pol, const float* host_in, uint32_t batch);
/* New parameters for an existing policy (a learner's update): `weights` as at rq_policy_create, repacked in place.  Precision, the
 * Standardize and SampleAndSquash stages and the current hidden state are kept; a resident executor is retired first.  Afterwards
 * every path computes what a policy freshly created with these weights computes, bit for bit. */
RQ_API int rq_policy_set_weights(rq_policy* pol, const float* weights, size_t n_weights);
/* Raptor over a SEQUENCE tensor, the layout rl-tools evaluates and the checkpoint's known-answer example
 * uses (checkpoint.h:197-215, [seq, batch, feature]): observation [steps, batch, obs_stride] (first 22
 * columns) -> action [steps, batch, 4].  Equivalent to `steps` calls of rq_policy_evaluate_step - the hidden
 * state is carried from the policy's current one and left after the last step - in ONE kernel launch
 * (operand image and GRU state stay in registers).  memory: RQ_DST_HOST = host arrays (copied, synchronous),
 * RQ_DST_DEVICE = device pointers (synchronised before return), RQ_DST_DEVICE_ASYNC = device pointers, only
 * enqueued on rq_device_stream(). */
RQ_API int rq_policy_evaluate_sequence(rq_policy* policy, const float* observation, uint32_t steps, uint32_t batch,
                                uint32_t obs_stride, float* action, int memory);

/* Known-answer self-test (README.md:136-139): runs `steps` x `batch` of a [steps,batch,22]
 * input through reset()+evaluate_step and reports max |out - expected|. */
RQ_API int rq_policy_selftest(rq_policy* pol, const float* input, const float* expected,
                       uint32_t steps, uint32_t batch, float tolerance, float* max_abs_err);

/* ---- Rollout: the loop body README.md:95-99, K times, on device ------------------------ */
typedef enum rq_rollout_mode {
    RQ_ROLLOUT_FUSED = 0,   /* one persistent kernel: state + hidden stay in registers for K steps */
    RQ_ROLLOUT_CHAINED = 1  /* observe -> evaluate_step -> step kernels, K x 3 launches (hipGraph)   */
} rq_rollout_mode;

enum rq_rollout_flags {
    RQ_ROLLOUT_AUTORESET = 1u  /* an env whose episode ends (terminated or step limit) is
                                  re-sampled in place (sample_initial_state + policy reset for
                                  that env) and keeps stepping; otherwise it freezes. */
};

/* Both modes leave the same state, hidden state, episode statistics and done codes, bit for bit.  The env's
 * device observation / action buffers (rq_env_get_observation / _action) are scratch of the chained mode only:
 * after a fused rollout they still hold what the last observe / evaluate_step call left there; use
 * rq_rollout_record to keep per-step observations and actions. */
RQ_API int rq_rollout(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state,
               rq_policy* policy, rq_rng* rng, uint32_t n_steps, int mode, uint32_t flags);

/* ---- Trajectory buffer: what a learner's data collection consumes (SURVEY.md section 8(f) row 1;
 * the reference's post_training collects ~77.7 k transitions per epoch, README.md:208).  A rollout
 * that records appends one entry per step and env: the 22 policy inputs, the raw action, the
 * reward and a done code (0 running, 1 terminated, 2 step limit reached, 4 env frozen = not
 * stepped; for code 4 the other fields are unspecified).  Device layout is step-major and
 * field-major inside a step (coalesced stores); rq_trajectory_get returns the learner layout
 * obs [T, N, 22], act [T, N, 4], rew [T, N], done [T, N]. */
typedef struct rq_trajectory rq_trajectory;
RQ_API int rq_trajectory_create(rq_env* env, uint32_t capacity_steps, rq_trajectory** out);
RQ_API int rq_trajectory_destroy(rq_trajectory* t);
RQ_API int rq_trajectory_reset(rq_trajectory* t);
RQ_API int rq_trajectory_length(const rq_trajectory* t, uint32_t* steps, uint32_t* capacity);
RQ_API int rq_trajectory_get(const rq_trajectory* t, float* obs, float* act, float* rew, uint8_t* done);
/* Relabel the recorded steps with `policy` (any policy object of this device, e.g. a teacher or a newer
 * student): actions of `policy` on the recorded observations, its GRU state
 * starting from the policy's current one (rq_policy_reset for episode starts), reset after recorded episode ends
 * (done 1/2) and held on frozen steps (done 4).  action_out: host [length, n_envs, 4] or NULL; overwrite != 0
 * also replaces the trajectory's stored actions.  With the policy that recorded the trajectory the result
 * equals the stored actions bit for bit. */
RQ_API int rq_trajectory_relabel(rq_trajectory* t, rq_policy* policy, float* action_out, int overwrite);
RQ_API int rq_trajectory_device_ptrs(const rq_trajectory* t, float** obs, float** act, float** rew,
                              uint8_t** done, uint32_t* ld);
RQ_API int rq_rollout_record(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state,
                      rq_policy* policy, rq_rng* rng, uint32_t n_steps, int mode, uint32_t flags,
                      rq_trajectory* trajectory);

/* ---- Tracking a moving setpoint (the reference environment's `trajectory` state component) ----
 * The policy is a position controller: it sees position and velocity relative to a target, and flies a path when it is fed
 * p - p_ref(t), v - v_ref(t).  A reference is a table host_rows [rows][6] of float32, row-major: columns 0..2 the target position,
 * columns 3..5 the target linear velocity, world frame (FLU).  The row an env uses at a step is ITS OWN episode step count at
 * observe time (rq_env_get_episode_steps before the step): every episode flies the path from its start, envs that reset at
 * different times are at different rows.  rq_reference_create refuses rows == 0 and non-finite entries.
 * rq_rollout_track is rq_rollout / rq_rollout_record (trajectory may be NULL) with ONE difference: after the observation is complete,
 * noise included, o[0..2] -= ref[k][0..2] and o[12..14] -= ref[k][3..5] (single fp32 subtractions) - what rq_observe, the same
 * subtraction on the host, rq_policy_evaluate_step and rq_step compute, bit for bit, in both modes.  Rotation matrix, body rates and
 * previous action are untouched; state, reward, termination thresholds, RNG streams and episode statistics stay on the ABSOLUTE
 * state - termination_position must contain the path.  A trajectory buffer records the shifted observation (what the policy saw),
 * so a tracked recording goes into rq_trajectory_relabel*, the learner and rq_trajectory_distill as it is.
 * Refused before anything is enqueued: a null argument, rows < episode_step_limit (no modulo: the table covers an episode), a
 * reference of another rq_device, a policy with a SampleAndSquash stage.  A teacher bank tracks through its own entry points
 * (rq_rollout_teachers_track, rq_rollout_teachers_track_refs).
 * Tracking error: per env, sum_sq = fp32 running sum of |p - ref[k][0..2]|^2 on the true (noise-free) position at observe time over
 * the steps actually taken (a frozen env adds nothing), steps = their count; both exist in tracked rollouts only, are the same bit
 * for bit in both modes, and are zeroed by rq_env_reset_statistics.  Either destination may be NULL. */
typedef struct rq_reference rq_reference;
RQ_API int rq_reference_create(rq_device* dev, const float* host_rows, uint32_t rows, rq_reference** out);
RQ_API int rq_reference_destroy(rq_reference* reference);
RQ_API int rq_rollout_track(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state,
                     rq_policy* policy, rq_rng* rng, uint32_t n_steps, int mode, uint32_t flags,
                     rq_trajectory* trajectory /* may be NULL */, const rq_reference* reference);
RQ_API int rq_env_get_tracking_error(const rq_env* env, float* sum_sq, uint32_t* steps, int dst_is_device);

/* ---- A suite of moving setpoints in one rollout: a reference per env ----
 * A reference bank is n_refs tables of the same length, host_rows [n_refs][rows][6] float32, columns as above.  In
 * rq_rollout_track_refs env i tracks table reference_id[i] (host array [n_envs]; ids are free per env, also inside a 64-env block)
 * and computes, bit for bit, what rq_rollout_track computes for it with a rq_reference made of that table: state and hidden state,
 * statistics and finished-episode records, done codes, the recording, the tracking-error sums and counts, the rng epoch moved on -
 * fused and chained, every precision, at a native interval, with noise, with or without auto-reset and recording.  The kernels are
 * rq_rollout_track's: they read row (reference_id[i] * rows + episode step count) of the flat table; the per-env first rows are
 * built from the ids on the host and cached on the device beside the env's tracking statistics, keyed by (bank, ids) - the same
 * ids upload nothing, other ids wait for the stream before the rows are rewritten.
 * rq_reference_bank_create refuses a null argument, n_refs == 0, rows == 0, a non-finite entry and n_refs * rows >= 2^28 (the row
 * index is a uint32).  The rollouts refuse, before anything is enqueued (state, rng epoch, statistics and recording untouched):
 * a null argument, a bank of another rq_device (RQ_ERR_SHAPE_MISMATCH), rows < episode_step_limit, an id >= n_refs (the message
 * names the env), a policy with a SampleAndSquash stage, and everything rq_rollout_track refuses. */
typedef struct rq_reference_bank rq_reference_bank;
RQ_API int rq_reference_bank_create(rq_device* dev, const float* host_rows /* [n_refs][rows][6] */, uint32_t n_refs, uint32_t rows,
                                    rq_reference_bank** out);
RQ_API int rq_reference_bank_destroy(rq_reference_bank* references);
RQ_API int rq_rollout_track_refs(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state,
                                 rq_policy* policy, rq_rng* rng, uint32_t n_steps, int mode, uint32_t flags,
                                 rq_trajectory* trajectory /* may be NULL */, const rq_reference_bank* references,
                                 const uint32_t* reference_id /* host [n_envs] */);

/* ---- Wrench schedule: scheduled gusts, pokes and payloads.  The per-episode constant wrench of the state (RQ_S_FORCE / RQ_S_TORQUE,
 * drawn at sample_initial_state) cannot express a gust from 1.5 s to 2.5 s, a one-step poke or a payload that hangs on from step 200.
 * A WRENCH BANK is n_tables tables of one length, host_rows [n_tables][rows][6] float32 row-major: columns 0..2 a force in the world
 * frame, 3..5 a torque in the body frame; `units` belongs to the bank: RQ_WRENCH_RELATIVE (force in multiples of m g, torque in
 * multiples of m g arm - the units of disturbance_force_std / disturbance_torque_std, meaningful across a domain-randomised
 * population) or RQ_WRENCH_ABSOLUTE (N and N m).  A schedule is attached to an ENV - a property of the world, not of who flies: a
 * bank plus one table id per env.  While it is attached EVERY transition of env i, in every call that steps (rq_step, the rollouts
 * of a policy, a policy bank and a teacher bank, fused or chained), is computed with the wrench
 *     k   = the env's episode step count before the step, clamped to rows - 1      (the count rq_rollout_track indexes with)
 *     row = table[wrench_id[i]][k]
 *     mg  = mass * gravity                        arm = sqrt((x0 * x0) + (y0 * y0))      x0, y0 = RQ_P_ROTOR_POS + 0, + 1
 *     fs  = relative ? mg : 1.0f                  ts  = relative ? mg * arm : 1.0f
 *     w[j]     = f[j]     + (fs * row[j])         j = 0..2     f = the state's RQ_S_FORCE / RQ_S_TORQUE (the per-episode draw)
 *     w[3 + j] = f[3 + j] + (ts * row[3 + j])
 * every *, + and sqrt one correctly rounded fp32 operation in this order, nothing contracted to an fma: NumPy float32 on the host
 * reproduces the bits (raptor_amd.disturbances.compose).  The schedule is never written into the state: RQ_S_FORCE / RQ_S_TORQUE of
 * the next state stay the per-episode base and a new episode's base is sampled as before; reward, termination, RNG streams,
 * statistics and observations are those of the resulting motion.  A frozen env reads nothing; rq_env_reset_statistics zeroes the
 * step count and so restarts the table; the scales come from the params passed to the call (rq_params_set after attaching is
 * honoured).
 * rq_wrench_bank_create refuses a null argument, n_tables == 0, rows == 0, a non-finite entry, n_tables * rows >= 2^28 and an
 * unknown `units`, all before the device is looked at.  rq_env_set_wrench_schedule (bank NULL: detach; wrench_id NULL: table 0 for
 * every env) refuses a bank of another rq_device (RQ_ERR_SHAPE_MISMATCH) and an id >= n_tables (the message names the env), waits
 * for the device's stream and uploads the per-env first rows once.  rq_wrench_bank_destroy is refused while the bank is attached
 * to a live env; rq_env_destroy detaches.  Every call that steps refuses, before anything is enqueued (state, rng epoch,
 * statistics and recording untouched), a bank with rows < episode_step_limit.  In fused mode a schedule is flown by the fp32
 * policy and policy-bank kernels (k_rollout_fused_wrench); a bf16 / f16x2 policy, a SampleAndSquash stage and rq_rollout_teachers*
 * are refused in fused mode while a schedule is attached (nothing runs chained in their place) - all three run chained.  The
 * small-batch loop steps such an env with plain launches (no resident executor, no speculative policy step). */
typedef struct rq_wrench_bank rq_wrench_bank;
enum rq_wrench_units { RQ_WRENCH_RELATIVE = 0, RQ_WRENCH_ABSOLUTE = 1 };
RQ_API int rq_wrench_bank_create(rq_device* dev, const float* host_rows /* [n_tables][rows][6] */, uint32_t n_tables, uint32_t rows,
                                 int units /* rq_wrench_units */, rq_wrench_bank** out);
RQ_API int rq_wrench_bank_destroy(rq_wrench_bank* bank);
RQ_API int rq_env_set_wrench_schedule(rq_env* env, rq_wrench_bank* bank /* NULL detaches */,
                                      const uint32_t* wrench_id /* host [n_envs] or NULL = table 0 */);
RQ_API int rq_env_get_wrench_schedule(const rq_env* env, rq_wrench_bank** bank /* NULL when none */,
                                      uint32_t* wrench_id_out /* host [n_envs] or NULL */);

/* ---- Vehicle schedule: the vehicle itself changes in mid-episode (a payload picked up or dropped, battery sag, a damaged propeller
 * set, slow motors).  A wrench schedule pushes on the vehicle; the mass, the inertia and the thrust the dynamics divide and multiply
 * by stay those of the params.  A VEHICLE BANK is n_tables tables of one length, host_rows [n_tables][rows][4] float32 row-major,
 * every entry a positive finite factor: column 0 the mass, 1 the inertia (all three axes), 2 the thrust curve (c0, c1, c2 alike),
 * 3 the motor time constant (rise and fall alike).  A schedule is attached to an ENV: a bank plus one table id per env.  While it
 * is attached EVERY transition of env i, in every call that steps (rq_step, the rollouts of a policy, a policy bank and a teacher
 * bank, chained; fused as said below), is computed from the EFFECTIVE parameters
 *     k    = the env's episode step count before the step, clamped to rows - 1   (the count the wrench schedule indexes with)
 *     row  = table[vehicle_id[i]][k]
 *     mass' = mass * row[0]
 *     Jxx' = Jxx * row[1]     Jyy' = Jyy * row[1]     Jzz' = Jzz * row[1]
 *     c0'  = c0 * row[2]      c1'  = c1 * row[2]      c2'  = c2 * row[2]
 *     tau_rise' = tau_rise * row[3]                   tau_fall' = tau_fall * row[3]
 *     every other field (rotor positions, torque constant, rpm range, hover rpm, hover action): the base value
 * every * one correctly rounded fp32 multiplication, nothing contracted.  The transition is the existing one on those 26 fields -
 * the per-env constants, reciprocals included, are made from the effective fields; the dynamics, reward, termination and counters
 * are unchanged: bit for bit what a caller gets who writes raptor_amd.vehicles.compose(P, row) with rq_params_set before every
 * rq_step.  Hence: a row of four 1.0f gives the unscheduled bits (x * 1.0f is x); the params object is never written - the base
 * values come from the params passed to the call, rq_params_set after attaching is honoured; a new episode's state is sampled from
 * the BASE parameters (mass, hover rpm); the reward's action baseline stays the base hover action; with a wrench schedule in
 * relative units attached as well the wrench scales use the step's effective mass (m g = mass' * gravity); a frozen env reads
 * nothing; rq_env_reset_statistics zeroes the step count and so restarts the table; whether an env's rotors rise and fall alike
 * is decided from tau_rise == tau_fall of the base fields (equal inputs times one factor are equal, and so are their reciprocals).
 * rq_vehicle_bank_create refuses a null argument, n_tables == 0, rows == 0, a factor that is not finite or not > 0 (the message names
 * table, row and column) and n_tables * rows >= 2^28, all before the device is looked at.  rq_env_set_vehicle_schedule (bank NULL:
 * detach; vehicle_id NULL: table 0 for every env) refuses a bank of another rq_device (RQ_ERR_SHAPE_MISMATCH) and an id >= n_tables
 * (the message names the env).  rq_vehicle_bank_destroy is refused while the bank is attached to a live env; rq_env_destroy
 * detaches.  Every call that steps refuses, before anything is enqueued (state, rng epoch, statistics and recording untouched), a
 * bank with rows < episode_step_limit.  In fused mode a schedule is flown by the fp32 policy and policy-bank kernels
 * (k_rollout_fused_vehicle); a bf16 / f16x2 policy, a SampleAndSquash stage, rq_rollout_teachers* and an env that carries a wrench
 * schedule too are refused in fused mode while a vehicle schedule is attached (nothing runs chained in their place) - all four run
 * chained.  The small-batch loop steps such an env with plain launches (no resident executor, no speculative policy step). */
typedef struct rq_vehicle_bank rq_vehicle_bank;
RQ_API int rq_vehicle_bank_create(rq_device* dev, const float* host_rows /* [n_tables][rows][4] */, uint32_t n_tables, uint32_t rows,
                                  rq_vehicle_bank** out);
RQ_API int rq_vehicle_bank_destroy(rq_vehicle_bank* bank);
RQ_API int rq_env_set_vehicle_schedule(rq_env* env, rq_vehicle_bank* bank /* NULL detaches */,
                                       const uint32_t* vehicle_id /* host [n_envs] or NULL = table 0 */);
RQ_API int rq_env_get_vehicle_schedule(const rq_env* env, rq_vehicle_bank** bank /* NULL when none */,
                                       uint32_t* vehicle_id_out /* host [n_envs] or NULL */);

/* ---- Wind schedule: the air moves, and the vehicle is dragged towards the air's velocity.  A wrench schedule applies a force that is
 * the same whatever the vehicle does; the force of wind depends on the vehicle's own velocity through the air: a quadrotor in a steady
 * wind leans into it and settles, one that drifts with the wind feels nothing, still air damps every motion.  A WIND BANK is n_tables
 * tables of one length, host_rows [n_tables][rows][4] float32 row-major: columns 0..2 the air velocity w in the world frame, m/s;
 * column 3 the specific drag d in 1/s, the drag force per unit mass and unit air speed (>= 0).  The drag is linear, the rotor-drag
 * regime of small multirotors.  A schedule is attached to an ENV: a bank plus one table id per env.  While it is attached EVERY
 * transition of env i, in every call that steps (rq_step, the rollouts of a policy, a policy bank and a teacher bank, chained; fused
 * as said below), is computed as
 *     k    = the env's episode step count before the step, clamped to rows - 1   (the count the other two schedules index with)
 *     row  = table[wind_id[i]][k]
 *     md   = mass * row[3]            mass: the params' RQ_P_MASS (with a vehicle schedule attached too: the step's effective mass)
 *     u[j] = row[j] - v[j]            j = 0..2, v = the linear velocity of the state BEFORE the step (state fields 7..9)
 *     w[j] = b[j] + (md * u[j])       b = the state's RQ_S_FORCE, or, with a wrench schedule attached too, the wrench-composed force
 *     torque: unchanged
 * every *, - and + one correctly rounded fp32 operation, in this order, nothing contracted (raptor_amd.winds.compose is the NumPy
 * float32 restatement).  The drag is a ZERO-ORDER HOLD: it is evaluated once, at the state entering the step, and held across the
 * four RK4 stages; it is not re-evaluated as the velocity changes inside the step.  At dt * d <= 0.01 * d this is benign for any
 * physical d, and it makes the transition bit for bit what a caller gets who writes this force into the state's force columns
 * before every rq_step.  The composed force goes to the dynamics and nowhere else.  Hence: the next state keeps the per-episode base
 * (RQ_S_FORCE is not written); a frozen env reads nothing; rq_env_reset_statistics zeroes the step count and so restarts the table;
 * the mass comes from the params passed to the call, rq_params_set after attaching is honoured; reward, termination, RNG streams,
 * statistics and observations are those of the resulting motion - the policy still sees the velocity over ground; a row with d = 0
 * adds +-0 to the force, which changes no bit of a base that is not -0.
 * rq_wind_bank_create refuses a null argument, n_tables == 0, rows == 0, an entry that is not finite, a negative drag (the message
 * names table, row and column) and n_tables * rows >= 2^28, all before the device is looked at.  rq_env_set_wind_schedule (bank NULL:
 * detach; wind_id NULL: table 0 for every env) refuses a bank of another rq_device (RQ_ERR_SHAPE_MISMATCH) and an id >= n_tables (the
 * message names the env).  rq_wind_bank_destroy is refused while the bank is attached to a live env; rq_env_destroy detaches.  Every
 * call that steps refuses, before anything is enqueued (state, rng epoch, statistics and recording untouched), a bank with rows <
 * episode_step_limit.  In fused mode a schedule is flown by the fp32 policy and policy-bank kernels (k_rollout_fused_wind); a bf16 /
 * f16x2 policy, a SampleAndSquash stage, rq_rollout_teachers* and an env that carries a wrench or a vehicle schedule too are refused
 * in fused mode while a wind schedule is attached (nothing runs chained in their place) - all of them run chained.  The small-batch
 * loop steps such an env with plain launches (no resident executor, no speculative policy step). */
typedef struct rq_wind_bank rq_wind_bank;
RQ_API int rq_wind_bank_create(rq_device* dev, const float* host_rows /* [n_tables][rows][4] */, uint32_t n_tables, uint32_t rows,
                               rq_wind_bank** out);
RQ_API int rq_wind_bank_destroy(rq_wind_bank* bank);
RQ_API int rq_env_set_wind_schedule(rq_env* env, rq_wind_bank* bank /* NULL detaches */,
                                    const uint32_t* wind_id /* host [n_envs] or NULL = table 0 */);
RQ_API int rq_env_get_wind_schedule(const rq_env* env, rq_wind_bank** bank /* NULL when none */,
                                    uint32_t* wind_id_out /* host [n_envs] or NULL */);

/* ---- Delay schedule: control latency.  Estimator, radio and ESC put one to several control periods between the actor's output and
 * the rotors' setpoint; the three schedules above change the force, the plant or nothing of the loop itself.  A DELAY BANK is
 * n_tables tables of one length, host_rows [n_tables][rows] uint8 row-major: the delay in steps, 0 <= d <= RQ_DELAY_MAX_STEPS (160 ms
 * at dt = 10 ms).  A schedule is attached to an ENV: a bank plus one table id per env.  While it is attached EVERY transition of env
 * i, in every call that steps (rq_step, the rollouts of a policy, a policy bank and a teacher bank, chained; fused as said below),
 * is computed as
 *     k    = the env's episode step count before the step, clamped to rows - 1   (the count the other schedules index with)
 *     d    = table[delay_id[i]][k]
 *     a_k  = the action given to the step: the policy's output, the teacher's, the caller's array in rq_step
 *     u_k  = a_{k-d} if d <= k, four +0.0f otherwise     (a command older than the episode is the zero sample_initial_state leaves
 *                                                          in the action history; d = 0: a_k itself)
 *     next state, reward, termination = those of the step computed from u_k, except
 *     RQ_S_LAST_ACTION of the next state = clamp(a_k, -1, 1), or a_k under action_history_raw
 * A controller sees what it sent, not what arrived: the observation's action history, a recording's actions (a_k), relabelling and
 * distillation all see the actor's own output (raptor_amd.delays.applied is the NumPy restatement of the rule; applied_actions
 * rebuilds u from a recording).  A table of zeros gives the bits of no schedule.
 * The env owns the COMMAND HISTORY: a ring on the device, allocated at the first attachment and kept, in which a step that commits
 * (not frozen) writes a_k at the slot of its episode step count.  It persists across calls: a step early in one call reads what the
 * call before wrote, whichever mode either flew in.  Attaching zeroes it - commands from before an attachment read as zero - and
 * an episode end or rq_env_reset_statistics needs no clearing, a command older than the episode being zero by the rule.
 * rq_delay_bank_create refuses a null argument, n_tables == 0, rows == 0, an entry above RQ_DELAY_MAX_STEPS (the message names table
 * and row) and n_tables * rows >= 2^28, all before the device is looked at.  rq_env_set_delay_schedule (bank NULL: detach, as
 * rq_env_clear_delay_schedule does; delay_id NULL: table 0 for every env) refuses a bank of another rq_device
 * (RQ_ERR_SHAPE_MISMATCH) and an id >= n_tables (the message names the env).  rq_delay_bank_destroy is refused while the bank is
 * attached to a live env; rq_env_destroy detaches.  Unlike the other schedules' banks, one with rows < episode_step_limit is flown:
 * the steps past the table hold its last row (constant latency is a table of one row).  In fused mode a schedule is flown by the
 * fp32 policy and policy-bank kernels (k_rollout_fused_delay); a bf16 /
 * f16x2 policy, a SampleAndSquash stage, rq_rollout_teachers* and an env that carries another schedule too are refused in fused mode
 * while a delay schedule is attached (nothing runs chained in their place, state, statistics, hidden state and history untouched) -
 * all of them run chained.  The small-batch loop steps such an env with plain launches (no resident executor, no speculative policy
 * step).  Not modelled: delays in fractions of a step, delays above RQ_DELAY_MAX_STEPS. */
#define RQ_DELAY_MAX_STEPS 16
typedef struct rq_delay_bank rq_delay_bank;
RQ_API int rq_delay_bank_create(rq_device* dev, const uint8_t* host_rows /* [n_tables][rows] */, uint32_t n_tables, uint32_t rows,
                                rq_delay_bank** out);
RQ_API int rq_delay_bank_destroy(rq_delay_bank* bank);
RQ_API int rq_env_set_delay_schedule(rq_env* env, rq_delay_bank* bank /* NULL detaches */,
                                     const uint32_t* delay_id /* host [n_envs] or NULL = table 0 */);
RQ_API int rq_env_clear_delay_schedule(rq_env* env);
RQ_API int rq_env_get_delay_schedule(const rq_env* env, rq_delay_bank** bank /* NULL when none */,
                                     uint32_t* delay_id_out /* host [n_envs] or NULL */);

/* ---- Sensor schedule: observation latency.  Motion capture over radio, or an onboard estimator slower than the controller, hands
 * the policy a state estimate that is one to several control periods old; the delay schedule above is the same on the command side.
 * A SENSOR BANK is n_tables tables of one length, host_rows [n_tables][rows] uint8 row-major: the delay in steps, 0 <= d <=
 * RQ_SENSOR_MAX_STEPS.  A schedule is attached to an ENV: a bank plus one table id per env.  While it is attached EVERY observation
 * assembled for env i (rq_observe, and every rollout of a policy, a policy bank and a teacher bank, chained; fused as said below) is
 *     k    = the env's episode step count as the observing kernel sees it (0 right after a reset or a thaw)
 *     z_k  = columns 0..17 of the observation as they are assembled without the schedule (position 0..2, rotation matrix 3..11,
 *            linear velocity 12..14, angular velocity 15..17), with the observation noise of that call's epoch, BEFORE any setpoint
 *            row is subtracted
 *     d    = table[sensor_id[i]][min(k, rows - 1)]           (a table shorter than an episode holds its last row)
 *     d'   = min(d, k)                                       (an episode younger than the delay sees its first reading held; it
 *                                                             never sees a reading of the episode before)
 *     delivered columns 0..17 = the stored bits of z_{k-d'}; columns 18..21 (the controller's own last command) and, in rq_observe's
 *            26-wide row, the rotor tail 22..25 are today's values
 * A tracked rollout subtracts the setpoint row of step k from the delivered columns (the controller knows the current setpoint); the
 * tracking error stays on the true position.  State and env step are unchanged; a recording holds what the policy saw
 * (raptor_amd.sensors.delivered is the NumPy restatement of the rule).  A table of zeros gives the bits of no schedule.
 * The env owns the READINGS: a ring on the device of 2 * RQ_SENSOR_MAX_STEPS slots x 18 fields x ld floats, slot k mod 32,
 * allocated at the first attachment and kept, zeroed at every attachment - readings from before an attachment read as zeros.  An
 * observation assembled at step k writes z_k to slot k for the envs inside the batch that are not frozen, then reads slot k - d'
 * where d' >= 1; the two never coincide.  Observing twice at one step rewrites the slot (with noise the later draw stands).  One
 * ring serves fused and chained launches and persists across calls, freezes and graph replays.
 * rq_sensor_bank_create refuses a null argument, n_tables == 0, rows == 0, an entry above RQ_SENSOR_MAX_STEPS (the message names
 * table and row) and n_tables * rows >= 2^28, all before the device is looked at.  rq_env_set_sensor_schedule (bank NULL: detach, as
 * rq_env_clear_sensor_schedule does; sensor_id NULL: table 0 for every env) refuses a bank of another rq_device
 * (RQ_ERR_SHAPE_MISMATCH) and an id >= n_tables (the message names the env).  rq_sensor_bank_destroy is refused while the bank is
 * attached to a live env; rq_env_destroy detaches.  Chained mode delivers with one small kernel over the env's observation buffer
 * (k_sensor_apply) behind every kernel that assembles an observation: every policy precision, the SampleAndSquash stage, teacher
 * banks and the four other schedules fly beside a sensor schedule there.  In fused mode the fp32 policy and policy-bank kernels fly
 * it (k_rollout_fused_sensor); a bf16 / f16x2 policy, a SampleAndSquash stage, rq_rollout_teachers* and an env that carries another
 * schedule too are refused in fused mode (nothing runs chained in their place; state, statistics, hidden state and readings
 * untouched).  The small-batch loop observes and steps such an env with plain launches (no observation cache, no mailbox rows, no
 * speculative policy step, no resident executor).  Not modelled: bias, scale, dropped readings, delays in fractions of a step,
 * per-column delays. */
#define RQ_SENSOR_MAX_STEPS 16
typedef struct rq_sensor_bank rq_sensor_bank;
RQ_API int rq_sensor_bank_create(rq_device* dev, const uint8_t* host_rows /* [n_tables][rows] */, uint32_t n_tables, uint32_t rows,
                                 rq_sensor_bank** out);
RQ_API int rq_sensor_bank_destroy(rq_sensor_bank* bank);
RQ_API int rq_env_set_sensor_schedule(rq_env* env, rq_sensor_bank* bank /* NULL detaches */,
                                      const uint32_t* sensor_id /* host [n_envs] or NULL = table 0 */);
RQ_API int rq_env_clear_sensor_schedule(rq_env* env);
RQ_API int rq_env_get_sensor_schedule(const rq_env* env, rq_sensor_bank** bank /* NULL when none */,
                                      uint32_t* sensor_id_out /* host [n_envs] or NULL */);

/* ---- Learner: the student's gradient over a recorded trajectory (README.md:208-216, the distillation step's regression) ----
 * Forward: the policy on the recorded observations obs [T][22][ld] under rq_trajectory_relabel's episode rules (GRU state back to
 * the learned initial state after done codes 1 and 2, held on code 4) -> action [T][4][ld_action] (ld_action >= n_envs; only the
 * columns of the n_envs envs are written, in every memory mode).  With
 * RQ_GRAD_START_CURRENT the first state is the policy's current one, a constant, and the actions equal rq_trajectory_relabel's bit
 * for bit; with RQ_GRAD_START_INITIAL it is the learned initial state (weights [2000:2016]) and its gradient counts.  The policy's
 * hidden state is not changed.  What the backward needs (the state entering each step, 64 B per env and step) stays in the
 * trajectory, tagged with the policy and its weights.
 * Backward: dL/da [T][4][ld_grad] -> grad_weights [2084] in the flat order (the initial state's slice included) and, optionally
 * and for RQ_GRAD_START_CURRENT only, grad_hidden_start [16][ld].  The exact gradient of the forward: ReLU'(0) = 0, actions of
 * frozen (code 4) steps depend on the parameters too, columns n_envs .. ld-1 contribute nothing whatever they hold.  Deterministic:
 * no float atomics, the same bits every run.  Refused (rq_last_error says which): no matching forward, weights changed since it
 * (rq_policy_set_weights, rq_policy_set_standardize), a bf16 / f16x2 policy, a Standardize or SampleAndSquash stage, objects of
 * two devices, an empty trajectory.  Gradients of those stages and of the observations are not computed.
 * memory: RQ_DST_HOST = host arrays (copied, synchronous), RQ_DST_DEVICE = device pointers (synchronised before return),
 * RQ_DST_DEVICE_ASYNC = device pointers, only enqueued on rq_device_stream(). */
enum rq_grad_start { RQ_GRAD_START_CURRENT = 0, RQ_GRAD_START_INITIAL = 1 };
RQ_API int rq_trajectory_policy_forward(rq_trajectory* t, rq_policy* policy, int start,
                                        float* action, uint32_t ld_action, int memory);
RQ_API int rq_trajectory_policy_backward(rq_trajectory* t, rq_policy* policy, const float* grad_action,
                                         uint32_t ld_grad, float* grad_weights, float* grad_hidden_start,
                                         int memory);

/* The distillation update without leaving the device.  The loss is the masked mean squared error between the policy's actions over
 * the recording (the forward above) and a target y [T][4][ld_target] (ld_target >= n_envs): the mean over the LIVE entries - done
 * code != 4, column < n_envs - of (a - y)^2, M = 4 x the live env-steps of them.  target == NULL: the trajectory's own stored
 * actions (what rq_trajectory_relabel_teachers(..., overwrite) or a teacher-acting rollout left there; ld_target is ignored).  What
 * is not live contributes nothing, whatever it holds (NaN in the targets or the observations of frozen steps included); M = 0 gives
 * loss 0 and a zero gradient.  No action or dL/da tensor is written or read: the backward recomputes the action from the state it
 * recomputes anyway, with the forward's own arithmetic.  Deterministic: no float atomics, the same bits every run.
 * rq_trajectory_policy_loss_grad: loss [1] and grad_weights [2084] = dloss/dtheta, no update.  Refusals and `memory` as for the
 * pair above (with RQ_DST_DEVICE* the target, loss and grad_weights are device memory of the trajectory's device; with RQ_DST_HOST
 * all three are host arrays).  It leaves the saved state of a forward behind: rq_trajectory_policy_backward may follow.
 * rq_optimizer: Adam's moments m, v [2084] and step count for ONE policy, zero at creation, with the hyper-parameters in device
 * memory.  The update is torch.optim.Adam's (bias-corrected moments, w -= lr m^ / (sqrt(v^) + eps)); weight_decay is decoupled
 * (w *= 1 - lr weight_decay first, torch.optim.AdamW's), 0 = none.  rq_optimizer_set_lr takes effect in stream order: updates
 * already enqueued keep the rate they were enqueued under.
 * rq_trajectory_distill: n_updates x (forward, loss-seeded backward, reduction, Adam, both fp32 operand images rebuilt on the
 * device), enqueued back to back on rq_device_stream() with no host synchronisation in between; losses [n_updates]: the loss
 * BEFORE each update.  With RQ_DST_DEVICE_ASYNC the call returns after enqueueing; whatever is enqueued on the same stream
 * afterwards - a rollout, a relabel - runs the updated policy.  The host's copy of the weights is refreshed (one 8 KB copy) by the
 * first call that needs it: rq_policy_get_weights, rq_policy_set_precision to a 16-bit precision, rq_policy_set_standardize,
 * rq_policy_selftest.  The policy's hidden state is kept.  Refused beyond the above: an optimizer made for another policy.
 * eps = 0 is accepted: an element whose v' is 0 (a gradient that has been exactly 0 since creation, m = v = 0) then updates by
 * 0 / (sqrt(0) + 0) = NaN, as torch.optim.Adam's does; with eps > 0 that element's update is exactly 0.
 * The state, for checkpointing a run and for driving the update directly:
 * rq_optimizer_get_state: m [2084], v [2084], step [1] (updates made so far) and beta_powers [2] = (beta1^step, beta2^step) as the
 * device carries them - running products, not recomputed powers - into host arrays, behind everything enqueued (as
 * rq_policy_get_weights).  rq_optimizer_set_state: the reverse from host arrays, bits copied, synchronous (it waits for the updates
 * enqueued).  The hyper-parameters are not part of the state: they are the rq_adam_config of rq_optimizer_create (and
 * rq_optimizer_set_lr).  A run restored - rq_policy_set_weights or a policy created from rq_policy_get_weights, an optimizer created
 * with the same config, rq_optimizer_set_state with what rq_optimizer_get_state gave - continues bit for bit: weights, moments,
 * step, powers and losses are those of the run that was never interrupted; that is why the two powers are taken, not step alone.
 * rq_optimizer_apply: ONE Adam update of the optimizer's policy from the caller's gradient grad [2084] (checkpoint order) - the
 * update of rq_trajectory_distill without its loss: rq_trajectory_policy_loss_grad followed by rq_optimizer_apply of that gradient
 * is, bit for bit, one rq_trajectory_distill update.  Both fp32 operand images are rebuilt and the host's copy of the weights, the
 * 16-bit images and a resident executor are made stale exactly as by rq_trajectory_distill.  memory: RQ_DST_HOST - grad is a host
 * array, the call returns when the update is done -, RQ_DST_DEVICE - device memory of the policy's device - or RQ_DST_DEVICE_ASYNC -
 * the same, only enqueued.  Refused before anything is enqueued, by all three: a null argument; an optimizer whose policy has been
 * destroyed; by rq_optimizer_apply also a `memory` outside the three, a gradient that is not where `memory` says, a policy that is
 * not the fp32 policy or has a Standardize stage. */
typedef struct rq_optimizer rq_optimizer;
typedef struct rq_adam_config { double lr, beta1, beta2, eps, weight_decay; } rq_adam_config;
RQ_API int rq_trajectory_policy_loss_grad(rq_trajectory* t, rq_policy* policy, const float* target, uint32_t ld_target,
                                          int start, float* loss, float* grad_weights, int memory);
RQ_API int rq_optimizer_create(rq_policy* policy, const rq_adam_config* config, rq_optimizer** out);
RQ_API int rq_optimizer_destroy(rq_optimizer* optimizer);
RQ_API int rq_optimizer_set_lr(rq_optimizer* optimizer, double lr);
RQ_API int rq_optimizer_get_state(rq_optimizer* optimizer, float* m, float* v, uint32_t* step, double* beta_powers /* [2] */);
RQ_API int rq_optimizer_set_state(rq_optimizer* optimizer, const float* m, const float* v, uint32_t step, const double* beta_powers);
RQ_API int rq_optimizer_apply(rq_optimizer* optimizer, const float* grad /* [2084] */, int memory);
RQ_API int rq_trajectory_distill(rq_trajectory* t, rq_policy* policy, rq_optimizer* optimizer, const float* target,
                                 uint32_t ld_target, int start, uint32_t n_updates, float* losses, int memory);
/* the policy's current parameters, 2 084 floats in the checkpoint order (after device-side updates: fetched from the device) */
RQ_API int rq_policy_get_weights(rq_policy* policy, float* host_out);

/* ---- Probes: what the GRU state knows about the quadrotor, and how early in an episode it knows it ----
 * Both calls read the state ENTERING every recorded step under the forward's episode rules from the learned initial state
 * (RQ_GRAD_START_INITIAL): the saved state a learner call above left in the trajectory if it was made by this policy at its current
 * weights with that start over the current length, else the forward is run first (its state-only form) and tagged.  The policy's own
 * hidden state is not changed.  Refusals as for rq_trajectory_policy_forward, and null pointers, before anything is enqueued.
 * rq_trajectory_get_hidden: out [length][n_envs][16], the learner layout.
 * rq_trajectory_probe_moments: targets y [n_targets][ld_targets], constant over time per env (1 <= n_targets <= 15, ld_targets >=
 * n_envs; columns >= n_envs are never read into a sum).  Per env an integer AGE: 0 at t = 0; a step is live when its done code is
 * not 4; a live step contributes the sample z = [1, h (16), y (n_targets), 0 ...] of D = 32 entries at its age; after a live step
 * with code 1 or 2 the age is 0 again, after any other live step it is one more; a frozen step changes and contributes nothing.
 * age_edges: host array [n_buckets + 1], strictly ascending, 1 <= n_buckets <= 32; a sample of age a belongs to bucket b when
 * age_edges[b] <= a < age_edges[b + 1], any other sample is dropped.  moments [n_buckets][32][32] doubles: per bucket the full
 * symmetric sum of z z^T (fp32 products and sums within a block of 64 envs, float64 across blocks); counts [n_buckets]: the samples.
 * Deterministic: no float atomics, the same bits every run.
 * memory: RQ_DST_HOST = targets, moments and counts are host arrays (targets checked finite in the envs' columns; synchronous);
 * RQ_DST_DEVICE / RQ_DST_DEVICE_ASYNC = device memory of the trajectory's device (synchronised before return / only enqueued on
 * rq_device_stream()); age_edges is a host array in every mode and is read before the call returns. */
RQ_API int rq_trajectory_get_hidden(rq_trajectory* t, rq_policy* policy, float* out, int memory);
RQ_API int rq_trajectory_probe_moments(rq_trajectory* t, rq_policy* policy,
                                       const float* targets, uint32_t ld_targets, uint32_t n_targets,
                                       const uint32_t* age_edges, uint32_t n_buckets,
                                       double* moments, uint64_t* counts, int memory);

/* TIMED MOMENTS: rq_trajectory_probe_moments for targets that change during an episode (the wrench of a scheduled gust, the velocity
 * of a moving setpoint).  Everything is as above except the targets: targets [length][n_targets][ld_targets] float32, length = the
 * trajectory's current length, and the sample of a live step t of env i is z = [1, h_t (16), targets[t][0 .. n_targets-1][i], 0 ...].
 * The age rule, the buckets and the dropped samples, D = 32, 1 <= n_targets <= 15, ld_targets >= n_envs, fp32 products and sums
 * inside a block of 64 envs and float64 across blocks in ascending block order, the full symmetric matrix and the counts are
 * unchanged.  A target value takes part in a sum only if its step is live, its age falls in a bucket and its column is below
 * n_envs; everything else (frozen steps, dropped ages, padding columns - NaN included) is selected away, never multiplied.  Targets
 * that do not change over time give the bits of rq_trajectory_probe_moments.  memory as above: RQ_DST_HOST copies the targets in
 * and first checks all length x n_targets x n_envs entries finite (the message names step, target and env); the device modes check
 * the pointers' device only.
 * WRENCH TARGETS: the scheduled wrench every env of a recording was flown with, rebuilt on the device from what decides it - a pure
 * function of the bank, one table id per env (wrench_id, host [n_envs]; NULL: table 0), the params, the episode step count of every
 * env when the recording began (start_steps, host uint32 [n_envs], what rq_env_get_episode_steps returned right before the rollout
 * that recorded step 0; NULL: all 0) and the recording's done codes.  out [length][6][ld_out]; per env, k = start_steps[i], and at
 * step t with done code d:
 *     d == 4: the six outputs are 0.0f, k stays
 *     else    row = table[wrench_id[i]][min(k, rows - 1)]
 *             units_out RQ_WRENCH_RELATIVE: out = row (refused for an RQ_WRENCH_ABSOLUTE bank)
 *             units_out RQ_WRENCH_ABSOLUTE: out[j] = fs * row[j], out[3 + j] = ts * row[3 + j], fs and ts as in "Wrench schedule"
 *                                           above from the params of this call (1.0f for an RQ_WRENCH_ABSOLUTE bank), one rounded
 *                                           fp32 product each
 *             then k = 0 if d is 1 or 2, else k + 1
 * This is the scheduled part of the wrench of that transition; the per-episode base (RQ_S_FORCE / RQ_S_TORQUE) is not part of it.
 * Bank and ids are arguments, not read from the env's attachment: that they are what was flown is the caller's business.  Columns
 * >= n_envs are not written.  wrench_id and start_steps are host arrays in every mode and are read before return; `memory` speaks
 * of `out`.  With RQ_DST_DEVICE_ASYNC this call and the moments chain on rq_device_stream() without a host synchronisation.
 * Refused before anything is enqueued, outputs untouched: a null trajectory, bank, params or out; an empty trajectory; a bank of
 * another device or params of another env (RQ_ERR_SHAPE_MISMATCH); an unknown units_out; relative output from an absolute bank;
 * ld_out < n_envs; rows < episode_step_limit; an id >= n_tables and start_steps[i] >= episode_step_limit (both name the env). */
RQ_API int rq_trajectory_probe_moments_timed(rq_trajectory* t, rq_policy* policy,
                                             const float* targets, uint32_t ld_targets, uint32_t n_targets,
                                             const uint32_t* age_edges, uint32_t n_buckets,
                                             double* moments, uint64_t* counts, int memory);
RQ_API int rq_trajectory_wrench_targets(rq_trajectory* t, const rq_wrench_bank* bank,
                                        const uint32_t* wrench_id /* host [n_envs] or NULL = table 0 */, const rq_params* params,
                                        const uint32_t* start_steps /* host [n_envs] or NULL = 0 */,
                                        int units_out /* rq_wrench_units */, float* out, uint32_t ld_out, int memory);

/* ---- Teacher bank: the distillation step of the reference (README.md:208-216: ~1000 teacher policies, one per
 * sampled quadrotor, queried on the states the student visited).  The teachers'
 * architecture is not in the reference tree - this is rl-tools' plain MLP family [UPSTREAM-UNVERIFIED]:
 *     input (first in_dim <= 22 recorded observation features) -> h1 -> h2 -> 4 actions,
 * h1, h2 in {16, 32, 64}, one activation for both hidden layers and one for the output.  Every env is labelled
 * by ITS teacher: envs are grouped by teacher id into 16-env tiles and each tile's three layers run as dense
 * contractions on the matrix cores with that teacher's operands held in registers for the whole trajectory. */
typedef enum rq_activation { RQ_ACT_IDENTITY = 0, RQ_ACT_RELU = 1, RQ_ACT_TANH = 2 } rq_activation;
typedef struct rq_teacher_bank rq_teacher_bank;
/* weights: n_teachers consecutive blocks [W1 (h1 x in_dim) | b1 (h1) | W2 (h2 x h1) | b2 (h2) | W3 (4 x h2) | b3 (4)],
 * matrices row-major with one row per output (the layout of rl-tools dense layers, checkpoint.h:39-53).
 * hidden_activation: RQ_ACT_RELU or RQ_ACT_TANH; output_activation: RQ_ACT_IDENTITY or RQ_ACT_TANH. */
RQ_API int rq_teacher_bank_create(rq_device* dev, const float* weights, uint32_t n_teachers, uint32_t in_dim,
                           uint32_t h1, uint32_t h2, int hidden_activation, int output_activation,
                           rq_teacher_bank** out);
/* Any sequential stack of dense layers - what a teacher checkpoint in the reference's HDF5 layout may hold (README.md:211-216;
 * raptor_amd.teachers.TeacherBank.from_checkpoints reads such files): in_dim -> widths[0] -> ... -> widths[n_hidden - 1] -> 4 with
 * n_hidden in 1..3 and widths multiples of 16 up to 128; weights: n_teachers blocks [W1 | b1 | ... | W_out (4 x last) | b_out].
 * Two hidden layers of 16 / 32 / 64 units are the register-stationary family above (this call then IS rq_teacher_bank_create);
 * everything else streams its fp32 operands from L2 through the exact-f32 MFMA (rq_teacher.hip k_teacher_relabel_layers):
 * rq_teacher_bank_set_precision accepts RQ_POLICY_FP32 only for such a bank. */
RQ_API int rq_teacher_bank_create_layers(rq_device* dev, const float* weights, uint32_t n_teachers, uint32_t in_dim,
                                  uint32_t n_hidden, const uint32_t* widths, int hidden_activation, int output_activation,
                                  rq_teacher_bank** out);
RQ_API int rq_teacher_bank_destroy(rq_teacher_bank* bank);
RQ_API int rq_teacher_bank_set_precision(rq_teacher_bank* bank, int precision);   /* rq_policy_precision */
/* Actions of teacher teacher_id[i] (host array, one id per env) on every recorded step of env i.
 * action_out: host [length, n_envs, 4] or NULL; overwrite != 0 replaces the trajectory's stored actions (what a
 * DAgger-style learner regresses on); otherwise they stay in a device scratch block (rq_trajectory_device_ptrs is
 * unaffected).  MLPs carry no state: done codes are not consulted, steps with code 4 get the teacher's action on
 * whatever observation is stored there. */
RQ_API int rq_trajectory_relabel_teachers(rq_trajectory* t, rq_teacher_bank* bank, const uint32_t* teacher_id,
                                   float* action_out, int overwrite);
/* Teacher teacher_id[i] on row i of a batch: the bank's counterpart of rq_policy_evaluate_step (a teacher has no state).
 * observation: host [batch, obs_stride] (obs_stride >= the teachers' in_dim; the first in_dim columns are read), or NULL: the env's
 * device observation buffer; action: host [batch, 4], or NULL: the env's device action buffer (rq_step / rq_rollout read it).  env
 * may be NULL when both are host arrays; otherwise batch must be the env's N_ENVIRONMENTS.  Every bank kind and precision.
 * The tile list built from teacher_id is cached in the bank: calls with the same ids upload nothing. */
RQ_API int rq_teacher_bank_evaluate(rq_teacher_bank* bank, rq_env* env, const uint32_t* teacher_id, const float* observation,
                                    uint32_t batch, uint32_t obs_stride, float* action);
/* The loop body README.md:95-99 x n_steps with env i flown by teacher teacher_id[i] of the bank: rq_rollout's semantics point for
 * point (observation noise by (rng epoch + step, env id), the epoch advanced by n_steps; statistics and finished-episode records;
 * RQ_ROLLOUT_AUTORESET re-samples in place, without it an ended env freezes and a later auto-reset rollout thaws it; done codes
 * 0 / 1 / 2 / 4).  trajectory: NULL, or a buffer of this env the rollout appends to - obs = the 22 policy-visible features, act =
 * the teacher's output after its output activation (before the env's clipping).
 * mode RQ_ROLLOUT_FUSED: one launch (rq_teacher_rollout.hip), fp32 banks of the two-hidden-layer {16, 32, 64} family only - a bf16 /
 * f16x2 bank or a dense stack is refused, never run chained in its place.  RQ_ROLLOUT_CHAINED: observe -> rq_teacher_bank_evaluate on
 * the env's buffers -> step per step, plain launches, every bank; fused and chained give the same bits.  Refused before anything is
 * enqueued (state, rng epoch, statistics and trajectory untouched): an id out of range, a bank / trajectory of another device or
 * env, a trajectory without room for n_steps, an unknown mode or flag, fused mode on a bank it does not run. */
RQ_API int rq_rollout_teachers(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state, rq_teacher_bank* bank,
                               const uint32_t* teacher_id, rq_rng* rng, uint32_t n_steps, int mode, uint32_t flags,
                               rq_trajectory* trajectory);
/* rq_rollout_teachers on a moving setpoint: rq_rollout_track's one difference (after the observation is complete, noise included, the
 * row of the env's own episode step count comes off the position and linear velocity the teacher sees; state, reward, termination and
 * statistics stay absolute; a trajectory records what the teacher saw, so rq_trajectory_relabel_teachers of a tracked recording
 * returns the recorded actions; rq_env_get_tracking_error accumulates over the steps actually taken) with env i flown by teacher
 * teacher_id[i].  A teacher has no state to hold: there is no native interval.  trajectory may be NULL.  Both modes, the banks each
 * mode runs as in rq_rollout_teachers (fused: one launch of the same kernel, tracking a wave-uniform switch; chained: the shift is a
 * launch of its own between the observation and the bank); fused and chained give the same bits.  Refused before anything is enqueued
 * (state, rng epoch, statistics and trajectory untouched), beside rq_rollout_teachers' refusals: a NULL reference
 * (RQ_ERR_INVALID_ARGUMENT), a reference of another device (RQ_ERR_SHAPE_MISMATCH), one with fewer rows than episode_step_limit
 * (RQ_ERR_INVALID_ARGUMENT). */
RQ_API int rq_rollout_teachers_track(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state, rq_teacher_bank* bank,
                                     const uint32_t* teacher_id, rq_rng* rng, uint32_t n_steps, int mode, uint32_t flags,
                                     rq_trajectory* trajectory /* may be NULL */, const rq_reference* reference);
/* The same with a reference bank: env i is flown by teacher teacher_id[i] on table reference_id[i] (host array
 * [n_envs]) - K teachers on M setpoints in one rollout.  Both id arrays are free per env, also inside a 16-env tile of one teacher.
 * Bit for bit rq_rollout_teachers_track with a rq_reference made of table r on the envs with reference_id[i] == r.  Refused as
 * rq_rollout_teachers_track and rq_rollout_track_refs refuse (an id >= n_refs: the message names the env). */
RQ_API int rq_rollout_teachers_track_refs(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state, rq_teacher_bank* bank,
                                          const uint32_t* teacher_id, rq_rng* rng, uint32_t n_steps, int mode, uint32_t flags,
                                          rq_trajectory* trajectory /* may be NULL */, const rq_reference_bank* references,
                                          const uint32_t* reference_id /* host [n_envs] */);

/* ---- Policy bank: many student policies in ONE rollout, one per wave.  Post-training writes a checkpoint per epoch and its
 * users pick the student by closed-loop return, episode length and share terminated; sweeps and seed populations ask the same
 * question.  A bank holds P policies of the Raptor topology (fp32; no Standardize stage, no SampleAndSquash stage; a native interval
 * per policy, 1 by default) as P operand images - the image rq_policy_pack_image returns for RQ_POLICY_FP32, slot after slot on the device - and a
 * rollout flies every aligned block of 64 envs with the policy named for it: a block is one wave, the weights are that wave's
 * MFMA operands, so 1 000 checkpoints x 64 quadrotors is one launch of 64 000 envs.
 * weights: [n_policies][2084], each block in the checkpoint order of rq_policy_create. */
typedef struct rq_policy_bank rq_policy_bank;
RQ_API int rq_policy_bank_create(rq_device* dev, const float* weights, uint32_t n_policies, rq_policy_bank** out);
RQ_API int rq_policy_bank_destroy(rq_policy_bank* bank);
/* New parameters for policy `index` (2084 floats): its slot is repacked in place, after the device's stream has drained; the
 * bank then computes what a bank created with these weights computes.  The hidden state stays. */
RQ_API int rq_policy_bank_set_weights(rq_policy_bank* bank, uint32_t index, const float* weights);
/* The bank's hidden state [n_envs, 16] is sized by the first rollout, as a policy's is by its first batch.  The initial state of
 * an env is its OWN policy's initial_hidden_state, so a reset is applied by the next use that knows the assignment: the next
 * rq_rollout_policies, or rq_policy_bank_get_hidden with the assignment of the last rollout.  rq_policy_bank_get_hidden before
 * the first rollout is RQ_ERR_NOT_INITIALIZED, with another batch than the last rollout's RQ_ERR_SHAPE_MISMATCH. */
RQ_API int rq_policy_bank_reset(rq_policy_bank* bank);
RQ_API int rq_policy_bank_get_hidden(rq_policy_bank* bank, float* host_out, uint32_t batch); /* [batch,16] */
/* The loop body README.md:95-99 x n_steps with env i flown by policy policy_id[i] (host array, one id per env) of the bank:
 * rq_rollout / rq_rollout_record's semantics point for point (observation noise by (rng epoch + step, env id), the epoch advanced
 * by n_steps; statistics and finished-episode records; RQ_ROLLOUT_AUTORESET re-samples in place and resets the env's policy state
 * to its policy's initial state, without it an ended env freezes and a later auto-reset rollout thaws it; done codes 0 / 1 / 2 /
 * 4).  trajectory: NULL, or a buffer of this env the rollout appends to.  What env i computes is, bit for bit, what rq_rollout
 * computes for it with a policy created from the weights of policy_id[i].
 * GRANULARITY IS THE WAVE: policy_id must be constant on every aligned block of 64 local env indices (the ragged last block is one
 * block); raptor_amd.policy_bank.block_policy_assignment deals blocks round-robin.
 * mode RQ_ROLLOUT_FUSED: one launch (k_rollout_fused_bank: k_rollout_fused with the image chosen per wave).  RQ_ROLLOUT_CHAINED:
 * observe -> actor step -> step (-> record) per step, plain launches; fused and chained give the same bits.  Refused before
 * anything is enqueued (state, rng epoch, statistics and trajectory untouched): an id >= n_policies or ids that differ inside a
 * block (RQ_ERR_INVALID_ARGUMENT), a bank / trajectory of another device or env (RQ_ERR_SHAPE_MISMATCH), a trajectory without
 * room for n_steps, an unknown mode or flag (RQ_ERR_INVALID_ARGUMENT).  The per-block id table is cached in the bank: calls with
 * the same ids upload nothing.  The bank's native intervals (below) are honoured.  Not offered with a bank: bf16 / f16x2, the
 * Standardize and SampleAndSquash stages, relabelling, the resident small-batch executors. */
RQ_API int rq_rollout_policies(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state, rq_policy_bank* bank,
                               const uint32_t* policy_id, rq_rng* rng, uint32_t n_steps, int mode, uint32_t flags,
                               rq_trajectory* trajectory);
/* Deployment control rate of a bank: rq_policy_set_native_interval's rule per policy - in every later rollout the hidden state of an
 * env flown by policy p moves on only at the steps whose episode step count is a multiple of interval[p], and the action of every
 * other step is computed from the last committed state (the first step of every episode is native).  interval: host array, n = 1
 * (one interval for every policy) or n = n_policies; each entry 1 .. RQ_POLICY_MAX_NATIVE_INTERVAL, anything else is refused
 * (RQ_ERR_INVALID_ARGUMENT, the message names the index) and changes nothing.  The call waits for the device's stream first, as
 * rq_policy_bank_set_weights does.  All intervals 1 (the default): every call does what it did before this entry point existed.
 * What env i computes is, bit for bit, what rq_rollout computes for it with a policy created from the weights of policy_id[i] and
 * set to interval[policy_id[i]] - policies of different intervals fly side by side in one launch (fused: k_rollout_fused_bank_rate,
 * the RATE loop with image and interval chosen per wave; chained: k_actor_step_rate_bank).  The bank's learner
 * (rq_trajectory_policies_loss_grad, rq_trajectory_policies_distill) is defined at the native rate only and refuses a bank with an
 * interval above 1.  rq_policy_bank_get_native_interval: out [n_policies]. */
RQ_API int rq_policy_bank_set_native_interval(rq_policy_bank* bank, const uint32_t* interval, uint32_t n);
RQ_API int rq_policy_bank_get_native_interval(const rq_policy_bank* bank, uint32_t* out); /* [P] */
/* rq_rollout_policies on a moving setpoint: rq_rollout_track's one difference (the row of the env's own episode step count comes off
 * the position and linear velocity the policy sees; state, reward, termination and statistics stay absolute; a trajectory records
 * what the policy saw; rq_env_get_tracking_error accumulates) with env i flown by policy policy_id[i] at its native interval.
 * trajectory may be NULL.  Refused before anything is enqueued, beside rq_rollout_policies' refusals: a NULL reference
 * (RQ_ERR_INVALID_ARGUMENT), a reference of another device (RQ_ERR_SHAPE_MISMATCH), one with fewer rows than episode_step_limit
 * (RQ_ERR_INVALID_ARGUMENT).  Bit for bit rq_rollout_track of the 64-env slices; fused and chained give the same bits. */
RQ_API int rq_rollout_policies_track(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state, rq_policy_bank* bank,
                                     const uint32_t* policy_id, rq_rng* rng, uint32_t n_steps, int mode, uint32_t flags,
                                     rq_trajectory* trajectory, const rq_reference* reference);
/* rq_rollout_policies_track with a reference bank: env i is flown by policy policy_id[i] at its native interval on table
 * reference_id[i] - P policies on M setpoints in one rollout.  policy_id is constant on every 64-env block; reference_id is free per
 * env.  Bit for bit rq_rollout_policies_track with a rq_reference made of table r on the envs with reference_id[i] == r.  Refused as
 * rq_rollout_policies_track and rq_rollout_track_refs refuse.  The teacher bank's twin: rq_rollout_teachers_track_refs. */
RQ_API int rq_rollout_policies_track_refs(rq_device* dev, rq_env* env, const rq_params* params, rq_state* state, rq_policy_bank* bank,
                                          const uint32_t* policy_id, rq_rng* rng, uint32_t n_steps, int mode, uint32_t flags,
                                          rq_trajectory* trajectory, const rq_reference_bank* references, const uint32_t* reference_id);

/* ---- Distilling a bank: the update of rq_trajectory_distill for every policy of a bank at once - a sweep of learning rates or a seed
 * population costs one student's launch count, and "fly the bank, distil the bank, fly it again" never leaves the device.  The
 * recording's 64-env blocks are dealt to the policies by policy_id as in rq_rollout_policies (host array, one id per env, constant
 * on every aligned block of 64); policy p's loss is the masked mean squared error of rq_trajectory_policy_loss_grad over ITS blocks
 * only, M_p = its live entries.  What policy p gets - loss, gradient, update - is, bit for bit, what a rq_policy created from its
 * weights gets from the single-policy calls on a recording that holds p's blocks alone, in order.
 * rq_trajectory_policies_loss_grad: loss [P], grad_weights [P][2084]; a policy that owns no block: loss NaN, its gradient row is
 * left as it was.  rq_bank_optimizer: Adam's state per policy, [P][2084] moments, and the hyper-parameters per policy: config
 * [n_cfg], n_cfg = 1 (one for all) or P; rq_bank_optimizer_set_lr: lr [n], n = 1 or P, in stream order.
 * rq_bank_optimizer_get_state / rq_bank_optimizer_set_state: rq_optimizer_get_state / _set_state for every policy at once - m, v
 * [P][2084], step [P], beta_powers [P][2], host arrays; a restored bank run continues bit for bit too.  Refused: a null argument, an
 * optimizer whose bank has been destroyed.  (There is no bank apply: the bank's update kernel is the single one's text.)
 * rq_trajectory_policies_distill: n_updates x (forward, loss-seeded backward, per-policy reduction, Adam and both operand images of
 * every policy), enqueued back to back; losses [n_updates][P]: the loss before each update.  A policy that owns no block in this
 * assignment is skipped whole - weights, moments, step count, images untouched - and its losses are NaN.  The updated weights are
 * what every later use of the bank on the same stream sees (a rollout, rq_policy_bank_get_hidden after a reset);
 * rq_policy_bank_get_weights fetches them ([P][2084], behind everything enqueued).
 * start, target, ld_target and memory as for the single-policy calls; RQ_GRAD_START_CURRENT reads the bank's hidden state, sized
 * for this env as by rq_rollout_policies, a pending reset applied first.  Refused before anything is enqueued: an id >= P or ids that
 * differ inside a block, a bank on another device, an optimizer made for another bank, n_updates = 0, an empty trajectory,
 * ld_target < n_envs, a target that is not device memory of the trajectory's device when one is announced. */
typedef struct rq_bank_optimizer rq_bank_optimizer;
RQ_API int rq_policy_bank_get_weights(rq_policy_bank* bank, float* host_out); /* [P][2084] */
RQ_API int rq_trajectory_policies_loss_grad(rq_trajectory* t, rq_policy_bank* bank, const uint32_t* policy_id, const float* target,
                                            uint32_t ld_target, int start, float* loss, float* grad_weights, int memory);
RQ_API int rq_bank_optimizer_create(rq_policy_bank* bank, const rq_adam_config* config, uint32_t n_cfg, rq_bank_optimizer** out);
RQ_API int rq_bank_optimizer_destroy(rq_bank_optimizer* optimizer);
RQ_API int rq_bank_optimizer_set_lr(rq_bank_optimizer* optimizer, const double* lr, uint32_t n);
RQ_API int rq_bank_optimizer_get_state(rq_bank_optimizer* optimizer, float* m, float* v, uint32_t* step, double* beta_powers);
RQ_API int rq_bank_optimizer_set_state(rq_bank_optimizer* optimizer, const float* m, const float* v, const uint32_t* step,
                                       const double* beta_powers);
RQ_API int rq_trajectory_policies_distill(rq_trajectory* t, rq_policy_bank* bank, rq_bank_optimizer* optimizer,
                                          const uint32_t* policy_id, const float* target, uint32_t ld_target, int start,
                                          uint32_t n_updates, float* losses, int memory);

/* ---- A weighted loss: the four loss calls above with a weight per env, or per env and step - hold out some envs of a recording and
 * report their loss (a 0/1 mask and its complement), trust good teachers more than bad ones, stress the first second after a reset.
 * weight: float32 [weight_steps][ld_weight], ld_weight >= n_envs; weight_steps = 1: one weight per env for every step; weight_steps
 * = the trajectory's length T: one per env and step, w[t][i].  Entry (t, i, k) - action k of env i at step t - COUNTS when it is live
 * (done code != 4, i < n_envs) and its weight is > 0.  Everything else is selected away, never multiplied: frozen steps, padding
 * columns, and weights that are 0, negative or NaN; NaN in the target, the observation or the weight of an entry that does not count
 * goes nowhere.  On a counting entry, in fp32 as the unweighted calls:
 *     e = a - y,   seed = fl(w e)  (dL/da before the scale),   term = fl(seed e),
 *     W4 = the sum of w over the counting entries (4 x the sum over the counting env-steps),
 *     loss = sum(term) / W4,   grad = (sum over the waves of their partial gradients) x 2 / W4.
 * Normaliser: W4 is accumulated in float64 - per lane over the lane's own entries in the order the kernel walks them, the 64 lanes of
 * a wave folded 0 .. 63, the waves in ascending order (for a bank: policy p's waves, W4_p) - and the scale is applied once, the
 * float64 product acc x (2 / W4) rounded to fp32 once; squared errors and partial gradients are reduced in wave order as in the
 * unweighted calls.  No float atomics: the same bits every run.  W4 = 0 (nothing counts) gives loss 0 and a zero gradient, not NaN;
 * the update then runs Adam on a zero gradient, which with zero moments and weight_decay = 0 leaves the weights as they are.  With
 * every weight 1.0f W4 is the integer M and each call returns the bits of its unweighted sibling: loss, gradient, updated weights.
 * Everything else - target == NULL meaning the stored actions, start, memory, the saved state a rq_trajectory_policy_backward may
 * follow, ordering on the stream, the optimizer belonging to the policy or bank, a policy of a bank that owns no block - is the
 * sibling's.  The weight travels like the target: RQ_DST_HOST copies a host array in, RQ_DST_DEVICE* take device memory of the
 * trajectory's device, which an enqueued-only call may still be reading when it returns.
 * Refused before anything is enqueued, outputs untouched (rq_last_error names the argument): a null weight; weight_steps that is
 * neither 1 nor T; ld_weight < n_envs; with RQ_DST_HOST a weight that is negative or not finite in the envs' columns (the message
 * names step and env - device memory is not read by the host: there such a weight drops its entries); a weight that is not device
 * memory of the trajectory's device when one is announced; and every refusal of the sibling. */
RQ_API int rq_trajectory_policy_loss_grad_weighted(rq_trajectory* t, rq_policy* policy, const float* target, uint32_t ld_target,
                                                   const float* weight, uint32_t ld_weight, uint32_t weight_steps, int start,
                                                   float* loss, float* grad_weights, int memory);
RQ_API int rq_trajectory_distill_weighted(rq_trajectory* t, rq_policy* policy, rq_optimizer* optimizer, const float* target,
                                          uint32_t ld_target, const float* weight, uint32_t ld_weight, uint32_t weight_steps,
                                          int start, uint32_t n_updates, float* losses, int memory);
RQ_API int rq_trajectory_policies_loss_grad_weighted(rq_trajectory* t, rq_policy_bank* bank, const uint32_t* policy_id,
                                                     const float* target, uint32_t ld_target, const float* weight,
                                                     uint32_t ld_weight, uint32_t weight_steps, int start, float* loss,
                                                     float* grad_weights, int memory);
RQ_API int rq_trajectory_policies_distill_weighted(rq_trajectory* t, rq_policy_bank* bank, rq_bank_optimizer* optimizer,
                                                   const uint32_t* policy_id, const float* target, uint32_t ld_target,
                                                   const float* weight, uint32_t ld_weight, uint32_t weight_steps, int start,
                                                   uint32_t n_updates, float* losses, int memory);

/* ---- Imitation error per env and episode age: how well the student imitates, as a table, from the forward alone - which teachers it
 * imitates badly (group the envs by teacher), how the error falls with episode age (the in-context adaptation curve), a held-out
 * loss without a backward, the error per setpoint, wrench scenario or policy of a sweep: all sums of this one table.
 * The actions a_t are those of rq_trajectory_policy_forward, bit for bit (the same step, the same episode rules, the same start);
 * the target y [T][4][ld_target] is the loss calls' (NULL: the trajectory's stored actions, ld_target ignored).  AGE is the probes':
 * 0 at the first recorded step; a step is live when its done code is not 4; after a live step with code 1 or 2 the age is 0 again,
 * after any other live step one more; frozen steps neither count nor age.  age_edges: host array [n_buckets + 1], strictly ascending,
 * 1 <= n_buckets <= 32, read before the call returns; a live step of age k belongs to bucket b when age_edges[b] <= k <
 * age_edges[b + 1], a live step outside every bucket is counted nowhere.  Per live step, in fp32, every operation rounded once and
 * none fused:  d_k = a_k - y_k,  e = ((d_0 d_0 + d_1 d_1) + d_2 d_2) + d_3 d_3.
 * sse [n_buckets][ld_out]: sse[b][i] = the sequential fp32 sum, in time order, of e over the steps of env i in bucket b (an env that
 * returns to a bucket in a later episode goes on from its total); count [n_buckets][ld_out]: the number of those steps.  ld_out >=
 * n_envs; every cell (b, i < n_envs) is written, columns >= n_envs are left as they were.  A frozen step, a step outside the buckets
 * and a padding column are selected away before any arithmetic: NaN in their targets or observations reaches no sum.  One lane sums
 * one env: no atomics, the same bits every run.  sum(sse) / (4 sum(count)) over all cells of edges {0, 2^32 - 1} is the masked MSE
 * of rq_trajectory_policy_loss_grad, summed in another order.
 * rq_trajectory_policies_error_table: the same for a bank, env i by policy policy_id[i] (host array, constant on every aligned block
 * of 64); a column block holds, bit for bit, what a rq_policy created from that policy's weights gives on it.
 * The calls read the recording and the policy and leave the trajectory's saved state alone: a rq_trajectory_policy_backward whose
 * forward came before the call may follow it and gives what it would have given without it.  The policy's hidden state is not changed.
 * memory: RQ_DST_HOST = target, sse and count are host arrays (synchronous); RQ_DST_DEVICE / RQ_DST_DEVICE_ASYNC = device memory of
 * the trajectory's device (synchronised before return / only enqueued on rq_device_stream()).
 * Refused before anything is enqueued, outputs untouched: every refusal of rq_trajectory_policy_loss_grad /
 * rq_trajectory_policies_loss_grad (a bf16 / f16x2 policy, a Standardize or SampleAndSquash stage, a native interval above 1,
 * objects of two devices, an empty trajectory, ld_target < n_envs, a target that is not device memory when one is announced, bad
 * ids); ld_out < n_envs; n_buckets outside 1 .. 32; edges that do not ascend strictly; a null argument; sse or count that is not
 * device memory of the trajectory's device when one is announced. */
RQ_API int rq_trajectory_policy_error_table(rq_trajectory* t, rq_policy* policy, const float* target, uint32_t ld_target,
                                            const uint32_t* age_edges, uint32_t n_buckets, int start, float* sse, uint32_t* count,
                                            uint32_t ld_out, int memory);
RQ_API int rq_trajectory_policies_error_table(rq_trajectory* t, rq_policy_bank* bank, const uint32_t* policy_id, const float* target,
                                              uint32_t ld_target, const uint32_t* age_edges, uint32_t n_buckets, int start,
                                              float* sse, uint32_t* count, uint32_t ld_out, int memory);

/* ---- Effective feedback gains per env and episode age: what the policy does with what it knows.  At every live recorded step, at
 * the recorded observation x (22) and the state h (16) entering the step, with the checkpoint's names
 *     p0 = W0 x + b0,  y0 = relu(p0),  m_k = [p0_k > 0]  (ReLU'(0) = 0),
 *     r = s(Wir y0 + bir + Whr h + bhr),  z = s(Wiz y0 + biz + Whz h + bhz),  c = Whn h + bhn,  n = tanh(Win y0 + bin + r c),
 *     h' = (1 - z) n + z h,  a = W2 h' + b2,
 *     A[i][k] = da_i/dp0_k = m_k sum_u W2[i][u] ((1 - z_u)(1 - n_u^2)(Win[u][k] + c_u r_u (1 - r_u) Wir[u][k])
 *                                              + (h_u - n_u) z_u (1 - z_u) Wiz[u][k]),
 * the instantaneous gain at fixed h is G = da/dx = A W0 [4][22] (columns: position 0..2, R row-major 3..11, linear velocity 12..14,
 * angular velocity 15..17, previous action 18..21).  The path of x_t into later actions through the recurrence is not part of it.
 * W0 is constant over the recording, so the calls sum A alone and the caller multiplies the sums by W0 once.  The step, the episode
 * rules and the start are those of rq_trajectory_policy_forward; AGE, age_edges and the buckets are those of the error table above.
 * sum [n_buckets][4][16][ld_out]: cell (b, i, k, e) = the sequential fp32 sum, in time order, of A_t[i][k] over the live steps of env
 * e whose age lies in bucket b (an env that returns to a bucket in a later episode goes on from its total); count
 * [n_buckets][ld_out]: the number of those steps.  ld_out >= n_envs; every cell with e < n_envs is written, columns >= n_envs are
 * left as they were.  A frozen step, a step outside the buckets and a padding column are selected away before any arithmetic on the
 * sums: NaN in a frozen observation reaches no sum.  One lane sums its own env's rows: no atomics, the same bits every run.
 * rq_trajectory_policies_gain_table: the same for a bank, env e by policy policy_id[e] (host array, constant on every aligned block
 * of 64); a column block holds, bit for bit, what a rq_policy created from that policy's weights gives on it.
 * The calls read the recording and the policy and leave the trajectory's saved state alone: a rq_trajectory_policy_backward whose
 * forward came before the call may follow it.  The policy's hidden state is not changed.  There is no target.
 * memory: RQ_DST_HOST = sum and count are host arrays (synchronous); RQ_DST_DEVICE / RQ_DST_DEVICE_ASYNC = device memory of the
 * trajectory's device (synchronised before return / only enqueued on rq_device_stream()).
 * Refused before anything is enqueued, outputs untouched, in the error table's words: a bf16 / f16x2 policy, a Standardize or
 * SampleAndSquash stage, a native interval above 1, objects of two devices, an empty trajectory, bad ids; ld_out < n_envs; n_buckets
 * outside 1 .. 32; edges that do not ascend strictly; a null argument; sum or count that is not device memory of the trajectory's
 * device when one is announced. */
RQ_API int rq_trajectory_policy_gain_table(rq_trajectory* t, rq_policy* policy, const uint32_t* age_edges, uint32_t n_buckets,
                                           int start, float* sum, uint32_t* count, uint32_t ld_out, int memory);
RQ_API int rq_trajectory_policies_gain_table(rq_trajectory* t, rq_policy_bank* bank, const uint32_t* policy_id, const uint32_t* age_edges,
                                             uint32_t n_buckets, int start, float* sum, uint32_t* count, uint32_t ld_out, int memory);

/* ---- Flight table: deviation, tilt and effort per env and episode age, read off a recording - how far a quadrotor was thrown, how
 * long it took to come back, how hard the motors worked and whether the commands hit their limits.  No policy takes part: the call
 * reads the recording alone, one pass that stores nothing of it.  With x the recorded observation of a step (x[0..2] the position
 * relative to the setpoint - under a moving setpoint too -, x[11] = R22 the cosine of the tilt, x[12..14] the linear and x[15..17]
 * the angular velocity, x[18..21] the previous action), a[0..3] the recorded action and r the recorded reward.
 * AGE: age = start_steps[i] at the first recorded step (host uint32 [n_envs], what rq_env_get_episode_steps returned right before
 * the rollout that recorded step 0; NULL: 0).  A step is live when its done code is not 4; after a live step with code 1 or 2 the age
 * is 0, after any other live step one more; a frozen step changes nothing and contributes nothing.  This is the row index of a
 * wrench schedule or a moving setpoint: a bucket of age is "time since the poke".  age_edges: host array [n_buckets + 1], strictly
 * ascending, 1 <= n_buckets <= 32; a live step of age k belongs to bucket b when age_edges[b] <= k < age_edges[b + 1], a live step
 * outside every bucket is counted nowhere.  start_steps and age_edges are host arrays in every mode and are read before return.
 * Per counted step, in fp32, every operation rounded once and none fused, sq3(p, q, s) = (p p + q q) + s s:
 *     RQ_FLIGHT_POS2       sq3(x0, x1, x2)
 *     RQ_FLIGHT_VEL2       sq3(x12, x13, x14)
 *     RQ_FLIGHT_OMEGA2     sq3(x15, x16, x17)
 *     RQ_FLIGHT_TILT       1.0f - x11
 *     RQ_FLIGHT_ACT2       sq3(a0, a1, a2) + a3 a3
 *     RQ_FLIGHT_DACT2      sq3(d0, d1, d2) + d3 d3,  d_k = a_k - x[18 + k]  (the change of command)
 *     RQ_FLIGHT_SATURATED  the number of k with |a_k| >= 1.0f, as a float (the env clips there)
 *     RQ_FLIGHT_OUTSIDE    1.0f where POS2 > tol2, else 0.0f;  tol2 = (float)tolerance * (float)tolerance, one fp32 product
 *     RQ_FLIGHT_REWARD     r
 * sum [n_buckets][RQ_FLIGHT_SUMS][ld_out]: cell (b, c, i) = the sequential fp32 sum s = s + v, in time order from 0.0f, of column c
 * over the steps of env i in bucket b (an env that returns to a bucket in a later episode goes on from its total).
 * peak [n_buckets][RQ_FLIGHT_PEAKS][ld_out]: the largest POS2, TILT and OMEGA2 of those steps, each from 0.0f by
 * p = v > p ? v : p, so a NaN never replaces a peak.  count [n_buckets][ld_out]: the number of those steps.
 * ld_out >= n_envs; every cell with column below n_envs is written, columns at or beyond n_envs are left as they were.  A frozen
 * step, a step outside the buckets and a padding column are selected away before any arithmetic: NaN there reaches no cell.  NaN
 * in a live, counted step goes into the cells of its own env and nowhere else.  One lane walks one env: no atomics, the same bits
 * every run.
 * memory speaks of sum, peak and count: RQ_DST_HOST = host arrays (synchronous); RQ_DST_DEVICE / RQ_DST_DEVICE_ASYNC = device memory
 * of the trajectory's device (synchronised before return / only enqueued on rq_device_stream()).
 * Refused before anything is enqueued, outputs untouched: a null trajectory, age_edges, sum, peak or count; an empty trajectory;
 * ld_out < n_envs; n_buckets outside 1 .. 32; edges that do not ascend strictly; a tolerance that is negative or not finite; an
 * unknown memory; sum, peak or count that is not device memory of the trajectory's device when one is announced. */
enum { RQ_FLIGHT_POS2, RQ_FLIGHT_VEL2, RQ_FLIGHT_OMEGA2, RQ_FLIGHT_TILT, RQ_FLIGHT_ACT2, RQ_FLIGHT_DACT2,
       RQ_FLIGHT_SATURATED, RQ_FLIGHT_OUTSIDE, RQ_FLIGHT_REWARD, RQ_FLIGHT_SUMS };      /* 9 */
enum { RQ_FLIGHT_PEAK_POS2, RQ_FLIGHT_PEAK_TILT, RQ_FLIGHT_PEAK_OMEGA2, RQ_FLIGHT_PEAKS }; /* 3 */
RQ_API int rq_trajectory_flight_table(rq_trajectory* t, const uint32_t* start_steps /* host [n_envs] or NULL = 0 */,
                                      float tolerance, const uint32_t* age_edges, uint32_t n_buckets,
                                      float* sum   /* [n_buckets][RQ_FLIGHT_SUMS][ld_out]  */,
                                      float* peak  /* [n_buckets][RQ_FLIGHT_PEAKS][ld_out] */,
                                      uint32_t* count /* [n_buckets][ld_out] */, uint32_t ld_out, int memory);


/* ---- Multi-GPU: the path's one exchange ---------------------------------------------
 * Envs are independent, so a batch shards over GPUs with no data-path collective: one process per GPU, rank r
 * owns the global env ids [r n, (r + 1) n) (rq_env_create's global_env_offset keys the RNG, results do not depend
 * on the sharding).  What is exchanged is the per-env return of the last finished episode: an RCCL all-gather
 * over xGMI, once per episode, in the C++ host.  Rank 0 obtains an id with rq_comm_unique_id and the host ships
 * its RQ_COMM_ID_BYTES bytes to the other ranks (MPI, a TCP store, a file - torch.distributed in bench.py); every
 * rank then calls rq_comm_create (a collective).  librccl is bound at run time (a copy the process already
 * mapped, e.g. PyTorch's, is shared; RQ_RCCL_LIBRARY overrides the search). */
#define RQ_COMM_ID_BYTES 128
typedef struct rq_comm rq_comm;
RQ_API int rq_comm_unique_id(void* id_out, size_t bytes);
RQ_API int rq_comm_create(rq_device* dev, uint32_t n_ranks, uint32_t rank, const void* id, size_t bytes, rq_comm** out);
RQ_API int rq_comm_destroy(rq_comm* comm);
/* (n_ranks, rank) as the communicator ITSELF reports them - ncclCommCount / ncclCommUserRank -, not rq_comm_create's arguments
 * handed back; rq_comm_create fails when the two disagree. */
RQ_API int rq_comm_info(const rq_comm* comm, uint32_t* n_ranks, uint32_t* rank);
/* What a record of a multi-GPU run needs to prove which RCCL saw how many ranks on which GPU (bench.py config.rccl):
 * every field is asked of RCCL / the HIP runtime at the time of the call. */
typedef struct rq_comm_description {
    uint32_t struct_bytes;        /* in: sizeof(rq_comm_description)                                                    */
    uint32_t n_ranks, rank;       /* ncclCommCount, ncclCommUserRank                                                    */
    int32_t  rccl_version;        /* ncclGetVersion (major * 10000 + minor * 100 + patch), -1 when the library has none  */
    int32_t  device;              /* ncclCommCuDevice: the HIP ordinal the communicator is bound to                      */
    char     pci_bus_id[32];      /* hipDeviceGetPCIBusId of that device, e.g. "0000:05:00.0"                            */
    char     library_path[256];   /* the file ncclAllGather was mapped from (dladdr): PyTorch's copy or /opt/rocm's      */
    uint64_t collectives_posted;  /* rq_allgather_returns calls on this communicator so far                             */
} rq_comm_description;
RQ_API int rq_comm_describe(const rq_comm* comm, rq_comm_description* out);
/* ENQUEUE the all-gather of this rank's rq_env_get_finished_returns: the copy on the env's own stream (right
 * behind the rollout that produced the returns), the collective on a side stream behind an event, double-
 * buffered; the host does not block.  Every rank must call it the same number of times with envs of the same size.
 * What "beside the next rollout" costs is measured in every default bench record (`native_exchange_1rank`: the real librccl
 * with one rank, an exchange posted after every 500-step launch with the next launch enqueued behind it; DESIGN.md
 * section 6): the fused kernel holds every SIMD, so the collective's own kernel starts as waves retire and the exchange
 * rides in the gap between two launches.  With N ranks the xGMI transfer of N x 4 B x n_envs comes on top; that part has
 * not run on hardware (one GPU per box). */
RQ_API int rq_allgather_returns(rq_env* env, rq_comm* comm);
/* Wait for the most recently enqueued all-gather: device pointer to the [n_ranks * n_envs] result in global env
 * order (valid until the second next rq_allgather_returns), its length, and optionally a host copy. */
RQ_API int rq_comm_gathered(rq_comm* comm, const float** dev_ptr, uint32_t* count, float* host_out);

/* ==== DIAGNOSTICS - not part of the drop-in boundary =======================================================================
 * Everything below is measurement instrumentation of THIS engine (bench.py, tools/): stopwatches, per-wave timing records of
 * the fused kernel, the launch floor, and the knobs of the small-batch loop.  No call site of the reference corresponds to any
 * of them and a reference-side binding would not bind them; they may change without an ABI bump
 * of the drop-in entry points above. */
/* HIP-event stopwatch on the device's own stream (what bench.py times kernels with). */
RQ_API int rq_device_timer_start(rq_device* dev);
RQ_API int rq_device_timer_stop(rq_device* dev, float* elapsed_ms);
/* Kernel-level timing of fused rollouts, off by default: while enabled every wave of a fused rollout kernel records the
 * wall-clock tick (constant 100 MHz) at which it came in and went out, and rq_device_last_rollout_ms returns, after waiting
 * for the most recent one, first-wave-in to last-wave-out on one die (the eight dies' counters are offset against one
 * another; the longest die counts).  rocprofv3's per-dispatch duration of the same launches (command processor takes the
 * dispatch -> the kernel's writes are released) reads a few microseconds more, by definition: bench.py carries both
 * (`roofline` / `roofline.wave_span`). */
RQ_API int rq_device_set_rollout_timing(rq_device* dev, int enable);
RQ_API int rq_device_last_rollout_ms(rq_device* dev, float* kernel_ms);
/* The records themselves (a diagnostic: tools/wave_timeline.py): per wave w of the most recent timed fused rollout four
 * ticks, records[4 w + 0] = the wave came in, [4 w + 1] = it went out (bits 0..59; bits 60..62 = the die (XCD) it ran on),
 * [4 w + 2] = its first step was about to start, [4 w + 3] = its last step was done; 100 MHz, comparable within one die
 * only.  `records` = NULL: *n_waves only; otherwise it holds 4 * capacity values. */
RQ_API int rq_device_last_rollout_waves(rq_device* dev, uint64_t* records, uint32_t capacity, uint32_t* n_waves);
/* The core clock (GHz) the most recent timed fused rollout ran its steps at: per wave, shader-clock cycles between its
 * first step's start and its last step's end over the same span in constant-rate ticks; the median over the waves that
 * stepped for at least a microsecond.  The clock follows the chip's load averaged over about a millisecond
 * (tools/idle_clock.py; measured: profiles/r04_idle_clock.txt), so a launch behind an idle gap runs slower than the same
 * launch in a busy loop.  (The three readers share one copy of the records per launch.) */
RQ_API int rq_device_last_rollout_clock(rq_device* dev, float* core_ghz);
/* Diagnostic: average time per launch (us, HIP events) of `reps` back-to-back launches of a kernel that only
 * stores one float per thread over n threads - what any standalone launch of that grid costs before it moves
 * its own data (bench.py reports it beside the API-granular kernels' HBM fractions). */
RQ_API int rq_device_launch_floor(rq_device* dev, uint32_t n, uint32_t reps, float* us_per_launch);
/* The small-batch loop's speculative policy step (README.md:96-99 at N < 1024 with host arrays): after a host-array
 * evaluate_step, every rq_step with a host action ALSO launches the policy the device last evaluated on the observation
 * the step just cached - next hidden state into a spare buffer of the policy, action rows into pinned memory - and the
 * following evaluate_step takes that result iff it is handed bit-identical rows, the same policy and an untouched policy
 * state.  Side effects a caller may see: one extra kernel launch per step on the device's stream, and the policy's
 * device-side action buffer overwritten by the speculated step.  A caller whose loop has another shape (perturbed
 * observations, alternating policies, env-only stepping) pays launches nobody uses: after 4 unused ones in a row the device
 * suspends speculation by itself and resumes when evaluate_step is again handed exactly the cached rows; enable = 0
 * switches it off for this device (RQ_NO_SPECULATION in the environment: off at rq_device_create), 1 on again.
 * rq_device_get_speculation: any out pointer may be NULL. */
RQ_API int rq_device_set_speculation(rq_device* dev, int enable);
/* The resident executor of that loop (round 6, ABI 5): once rq_step has been called three times in a row, each within 200 us of the one
 * before, in the loop's own shape (host actions, an env of at most 256 envs, the observation cached, an fp32 policy to speculate with,
 * next_state != state) and nothing else was asked of the device in between, the step and the speculated policy step are no longer
 * LAUNCHED: one workgroup stays on the device, on a stream of its own, polls a 64-byte command line (pinned host memory, or device memory
 * behind a large BAR) and does for every command what the two launches did (same device functions, same bits, same sequence numbers in
 * the same flag).  Any other call on the device retires it first (a few microseconds); it leaves by itself after 300 us without a
 * command and, between two commands, once it is 1 ms old (a device-wide synchronize waits for a running kernel); a command it never
 * took is replayed as launches; kernels that idle out having served fewer than 8 commands are started 8, 16, ... 1 024 steps apart.
 * A loop paced like README.md:94-101 (10 ms of sleep per step) keeps its launches.  Results never depend on any of this.  enable = 0
 * switches it off for this device (RQ_NO_RESIDENT in the environment: off at rq_device_create); either value clears the back-off.
 * The same executor serves a policy ALONE: rq_policy_evaluate_step with host rows (env = NULL), at most 16 of them, an fp32 policy
 * without a sampling stage, called three times in a row within 200 us of one another (README.md:17-25, a caller with a simulator of
 * its own) - from then on the rows are commands to a resident wave that keeps the hidden state in registers (and in the policy's buffer,
 * every step); same lifecycle, same bits as the launch.  One resident kernel per device at a time, of either kind.
 * rq_device_get_resident: any out pointer may be NULL; `running` = a kernel is on the device now; starts / commands / replays count
 * kernels started, commands posted, and commands replayed as launches since the device was created (both kinds). */
RQ_API int rq_device_set_resident(rq_device* dev, int enable);
RQ_API int rq_device_get_resident(const rq_device* dev, int* enabled, int* running, uint64_t* starts, uint64_t* commands, uint64_t* replays);
/* Six device timestamps (100 MHz ticks) of the last command the resident kernel finished: command seen, action rows read, env stepped
 * (observation rows written), first sequence number published, policy evaluated (action rows written), second number published. */
RQ_API int rq_device_get_resident_timing(const rq_device* dev, uint64_t* ticks6);
RQ_API int rq_device_get_speculation(const rq_device* dev, int* enabled, int* suspended, uint32_t* consecutive_misses);

#ifdef __cplusplus
}
#endif
#endif /* RAPTOR_QUAD_H */
