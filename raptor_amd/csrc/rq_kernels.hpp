// rq_kernels.hpp — host-visible interface of the HIP kernels (internal to libraptor_quad.so).
// POD argument blocks are passed to the kernels by value (they land in SGPRs via the kernarg
// segment); pointers are device pointers to field-major struct-of-arrays buffers.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "../../include/raptor_quad.h"
#include "rq_fused_route.hpp"
#include "rq_loss_launch.hpp"
#include "rq_step_launch.hpp"      // StepCfg, NoiseCfg, SampleCfg, StatsPtrs, WrenchPtrs, SasArgs, Batch, Mailbox; the chained step's launches

namespace rq {

inline StepCfg step_cfg(const rq_env_config& c) {
    return {c.dt, c.gravity, c.episode_step_limit, c.reward_scale, c.reward_constant,
            c.reward_termination_penalty, c.reward_position, c.reward_orientation,
            c.reward_linear_velocity, c.reward_angular_velocity, c.reward_action,
            c.termination_enabled, c.termination_position, c.termination_linear_velocity,
            c.termination_angular_velocity, c.action_history_raw};
}
inline NoiseCfg noise_cfg(const rq_env_config& c) {
    return {c.noise_position, c.noise_orientation, c.noise_linear_velocity, c.noise_angular_velocity};
}
inline bool noise_enabled(const rq_env_config& c) {
    return c.noise_position > 0.f || c.noise_orientation > 0.f || c.noise_linear_velocity > 0.f ||
           c.noise_angular_velocity > 0.f;
}
inline SampleCfg sample_cfg(const rq_env_config& c) {
    return {c.gravity, c.domain_randomization, c.dr_scale_min, c.dr_scale_max,
            c.dr_thrust_to_weight_min, c.dr_thrust_to_weight_max, c.dr_torque_const_min,
            c.dr_torque_const_max, c.dr_motor_tau_min, c.dr_motor_tau_max, c.init_guidance,
            c.init_max_position, c.init_max_angle, c.init_max_linear_velocity,
            c.init_max_angular_velocity, c.disturbance_force_std, c.disturbance_torque_std};
}

// Trajectory buffer of a rollout: step-major, field-major within a step,
//   obs [T][22][ld], act [T][4][ld] (raw actor output), rew [T][ld], done [T][ld] (codes of last_done).
struct TrajPtrs {
    float* obs; float* act; float* rew; uint8_t* done;
    uint32_t t0;          // index of the first step this launch writes
};

// A tracked rollout (rq_rollout_track): the reference table and the env's two tracking statistics.
struct TrackPtrs {
    const float* ref;     // [rows][6] row-major: target position, target linear velocity (world frame); nullptr = untracked
    uint32_t rows;
    // A reference bank (rq_rollout_track_refs): `ref` is M tables one after another, [M * rows][6], and env i reads the table that
    // begins at row steps[row0_at + i] = reference_id[i] * rows - per lane, with no wave granularity: the row was a per-lane gather
    // already.  The env's tracking block holds that [ld] array behind the counts.  0 (wave-uniform: a kernel argument) = every env's
    // table begins at row 0, the single reference.  An offset in what was the struct's padding, not a pointer: the RATE kernels take
    // TrackPtrs by value in their TRACK = false instantiations too, and a struct that grew would move their argument block.
    uint32_t row0_at;
    float* sq;            // [ld]: running sum of |p - p_ref|^2 over the steps taken
    uint32_t* steps;      // [ld]: how many
};
static_assert(sizeof(TrackPtrs) == 32, "the kernels' argument blocks hold TrackPtrs by value");

// ---- resident executor of the small-batch loop (rq_kernels.hip k_resident_loop; host side: rq_capi_vector.cpp resident_*) ----
struct ResidentArgs {
    Batch b; StepCfg c; SampleCfg sc; uint64_t seed;
    const float* params; float* act; StatsPtrs st;
    float* obs_buf[2];            // the env's two observation buffers; a command's bit 0 picks the one this step writes
    const float* packed;          // the policy's f32 operand image
    float* hidden[2];             // the policy's two hidden-state buffers; bit 1 picks the one that is read (the other is written)
    uint32_t ld_h; float* pol_act;
    const float* rows_action;     // pinned: [n][4] actions of the command
    const uint32_t* small_rows;   // pinned: the same rows once more, 48 dwords right where the poll of k_resident_small reads them (n <= 12)
    float* rows_obs;              // pinned: [n][RQ_OBSERVATION_DIM] observation of the state the step wrote
    float* rows_act;              // pinned: [n][4] the policy's actions on that observation
    uint32_t* flag;               // pinned: the device's mailbox flag (sequence numbers of finished work)
    volatile uint32_t* packet;    // pinned: 16 dwords, see ResidentPacket
    uint32_t* exited;             // pinned: [0] receives launch_id when the kernel has left, [1] why (0 told to, kRbLeftIdle, kRbLeftOld)
    unsigned long long* timing;   // pinned: six 100 MHz timestamps of the last command (seen, rows read, stepped, first flag, acted, done)
    uint32_t launch_id, first_packet;
    unsigned long long idle_ticks;       // 100 MHz ticks without a command after which the kernel leaves
    unsigned long long life_ticks;       // ... and its age at which it leaves between two commands whatever the traffic (the host starts another)
};
// dwords of the command line (one 64-byte line of pinned host memory, written body first, then tail, then head)
enum ResidentPacket { kRpHead = 0, kRpBits = 1, kRpStateInLo = 2, kRpStateInHi = 3, kRpStateOutLo = 4, kRpStateOutHi = 5,
                      kRpSeqStep = 6, kRpSeqSpec = 7, kRpChecksum = 8, kRpTail = 15 };
constexpr uint32_t kResidentSmallEnvs = 12;      // 4 n action dwords fit the 48 lanes the command line leaves of one poll
enum ResidentBits : uint32_t { kRbObsSel = 1u, kRbHiddenSel = 2u, kRbQuit = 4u,
                               kRbLeftIdle = 8u, kRbLeftOld = 16u };      // set by the kernel itself: why it left (exited[1])

constexpr uint32_t kResidentPolicyBatch = 16;    // the policy-only executor: one 16-env tile
constexpr uint32_t kResidentPolicyRow = 24;      // floats per observation row in command memory (22 + padding to whole 16-byte words)

// one workgroup of ceil(n / 64) <= 4 waves on stream s; returns at once, the kernel stays until told to quit or idle for idle_ticks
hipError_t launch_resident(hipStream_t s, const ResidentArgs& ra);
// the policy alone (rq_policy_evaluate_step with host rows, batch <= kResidentPolicyBatch): uses packed, hidden[0] (in place), ld_h,
// pol_act, small_rows (observation rows [n][kResidentPolicyRow] behind the command line), rows_act, flag, packet, exited; b.n = batch
hipError_t launch_resident_policy(hipStream_t s, const ResidentArgs& ra);

// vector.sample_initial_parameters (README.md:60)
hipError_t launch_sample_params(hipStream_t s, Batch b, SampleCfg c, uint64_t seed, uint32_t epoch, float* params);
// vector.sample_initial_state (README.md:61): uses episode[i] as the RNG counter, increments it, unfreezes the
// env and starts its running return / step count at zero (a new episode begins)
hipError_t launch_sample_state(hipStream_t s, Batch b, SampleCfg c, uint64_t seed, const float* params,
                               float* state, StatsPtrs st);
// vector.observe (README.md:96): obs [RQ_OBSERVATION_DIM][ld]
// epoch used = epoch + (epoch_base ? *epoch_base : 0): epoch_base is a device counter for launches
// replayed from a hipGraph (see rq_rollout, chained mode)
hipError_t launch_observe(hipStream_t s, Batch b, NoiseCfg nc, bool noise, uint64_t seed, uint32_t epoch,
                          const uint32_t* epoch_base, const float* params, const float* state, float* obs,
                          Mailbox mb = Mailbox{});
// ---- explicit hipGraph construction (round 6) -------------------------------------------------------------------------------------
// A chained rollout replays a graph of kGraphSteps steps.  Rounds 2-5 built it by STREAM CAPTURE - and while any stream of a process
// captures, HIP fails hipDeviceSynchronize (and other calls) on EVERY thread of the process with hipErrorStreamCaptureUnsupported and
// invalidates the capture: a learner's PyTorch thread on the same GPU both broke the rollout and was broken by it (measured:
// tools/foreign_soak.py).  Now the graph is built node by node: while a GraphSink is installed on the calling thread, the launchers a
// chained step uses (launch_actor_step, launch_step, launch_add_u32) append a kernel node - same kernel, same grid, same arguments,
// each depending on the one before - instead of launching.  No stream is ever in capture mode.
struct GraphSink {
    hipGraph_t graph = nullptr;
    hipGraphNode_t last = nullptr;
    hipError_t status = hipSuccess;
    uint32_t nodes = 0;
};
void set_graph_sink(GraphSink* sink);      // nullptr: the launchers launch again (thread-local)

hipError_t launch_set_u32(hipStream_t s, uint32_t* p, uint32_t value);
hipError_t launch_add_u32(hipStream_t s, uint32_t* p, uint32_t add);
// The chained step's three launches, each from its description (rq_step_launch.hpp: the fields say what they mean).  The actor
// step and the env step append a node under a GraphSink, the thaw launches.
// launch_actor_step: Raptor.evaluate_step (README.md:97) of one policy or a policy bank, by the kernel route_actor_step names for
// actor_step_traits(a) - hipErrorInvalidValue, and nothing launched, for a description no kernel is built for.
hipError_t launch_actor_step(hipStream_t s, const ActorStepLaunch& a);
// Raptor over a sequence: obs [steps][n][stride] (first 22 columns) -> act [steps][n][4], both row-major on
// the device; hidden [16][ld_h] is the state before step 0 on entry and after the last step on return
hipError_t launch_actor_sequence(hipStream_t s, uint32_t n, uint32_t steps, const float* packed, const float* obs,
                                 uint32_t stride, float* hidden, uint32_t ld_h, float* act, int precision);
// a policy over a recorded trajectory: obs [steps][22][ld], done [steps][ld] -> act [steps][4][ld] (field-major),
// GRU state reset after done codes 1/2, held on code 4; hidden [16][ld_h] in/out
hipError_t launch_actor_relabel(hipStream_t s, uint32_t n, uint32_t ld, uint32_t steps, const float* packed,
                                const float* obs, const uint8_t* done, float* hidden, uint32_t ld_h, float* act,
                                int precision);
// The learner (rq_grad.hpp).  Forward: launch_actor_relabel's pass over obs [steps][22][ld] / done [steps][ld] with the state
// entering each step saved to `saved` [steps][16][ld]; it starts from hidden [16][ld_h] (start_initial = 0) or the learned initial
// state, writes act [steps][4][ld_act] and leaves `hidden` alone.  Backward: dL/da [steps][4][ld_g] -> per-wave partial gradients
// partial [ceil(n / 64)][2084] (flat weight order) and dL/dh_start [16][ld] (grad_h_start, may be null; start_initial = 0 only),
// then a fixed-order sum of the partials into grad [2084].  `gpacked`: the transposed image (pack_policy_grad).
hipError_t launch_policy_grad_forward(hipStream_t s, uint32_t n, uint32_t ld, uint32_t steps, const float* packed,
                                      const float* obs, const uint8_t* done, const float* hidden, uint32_t ld_h,
                                      int start_initial, float* act, uint32_t ld_act, float* saved);
hipError_t launch_policy_grad_backward(hipStream_t s, uint32_t n, uint32_t ld, uint32_t steps, const float* packed,
                                       const float* gpacked, const float* obs, const uint8_t* done, const float* saved,
                                       const float* grad_act, uint32_t ld_g, int start_initial, float* grad_h_start,
                                       float* partial, float* grad);
// The distillation update on the device (rq_grad.hpp, rq_grad_bank.hpp).  launch_policy_loss_grad: every form of the loss launch -
// one policy or a bank, weighted or not - as rq_loss_launch.hpp's LossLaunch describes it.  Deterministic.
hipError_t launch_policy_loss_grad(hipStream_t s, const LossLaunch& a);
// its first launch alone: the forward that saves the state and stores no action (the probes read nothing else); what it does not
// read of the description - the transposed image, the target, the weight, the workspace, the outputs - may stay unset
hipError_t launch_policy_grad_forward_state(hipStream_t s, const LossLaunch& a);
// The forward alone, storing nothing of the pass: the squared imitation error per env and bucket of episode age, one policy or a bank,
// as rq_loss_launch.hpp's ErrorTableLaunch describes it.  One launch; a lane sums its own env: deterministic, no atomics.
hipError_t launch_policy_error_table(hipStream_t s, const ErrorTableLaunch& a);
// The backward's recompute walked forwards with four local seeds: A = da/dp0 [4][16] summed per env and bucket of episode age, one
// policy or a bank, as rq_loss_launch.hpp's GainTableLaunch describes it.  One launch; a lane sums its own rows: deterministic.
hipError_t launch_policy_gain_table(hipStream_t s, const GainTableLaunch& a);
// Adam's state on the device: hyper-parameters, the step count t and the running powers beta^t (1 before the first step)
struct AdamState { double lr, beta1, beta2, eps, weight_decay, beta1_t, beta2_t; uint32_t step, pad; };
// one element of an operand image as a function of the flat weights: 0 (a == PACK_GATHER_NONE), k w[a], or k (w[a] + w[b])
struct PackGather { uint16_t a, b; float k; };
enum { PACK_GATHER_NONE = 0xFFFF };
// one Adam step on w / m / v [2084] from grad, then packed (pack_policy's image) and gpacked (pack_policy_grad's) rebuilt from the
// new weights through table [RQ_PACKED_FLOATS + RQ_PACKED_GRAD_FLOATS] (pack_gather_table)
hipError_t launch_adam_repack(hipStream_t s, const float* grad, float* w, float* m, float* v, AdamState* st, const PackGather* table,
                              float* packed, float* gpacked);
hipError_t launch_adam_set_lr(hipStream_t s, AdamState* st, double lr);
// The bank's (rq_grad_bank.hpp).  launch_adam_repack_bank: one Adam step per policy that owns a wave (wave_offsets [P + 1], the CSR
// list of the loss launch), on w / m / v [P][2084] with st [P], and both its images rebuilt.  launch_adam_set_lr_bank: lr [n_lr], n_lr
// = 1 (for all) or P, a host array read before the call returns.
hipError_t launch_adam_repack_bank(hipStream_t s, uint32_t n_policies, const uint32_t* wave_offsets, const float* grad, float* w, float* m,
                                   float* v, AdamState* st, const PackGather* table, float* images, float* gimages);
hipError_t launch_adam_set_lr_bank(hipStream_t s, AdamState* st, uint32_t n_policies, const double* lr, uint32_t n_lr);
// dst [rows][ld] <- src [rows] (device), row by row
hipError_t launch_fill_rows(hipStream_t s, float* dst, uint32_t ld, const float* src, uint32_t rows);
// launch_step: vector.step (README.md:98) + reward / termination / statistics, with a rollout's episode-end handling, host rows,
// the folded observation and a wrench schedule as the description asks; a bank's step (block_policy set) is a rollout's, in place,
// without host rows or a folded observation - anything else: hipErrorInvalidValue.
hipError_t launch_step(hipStream_t s, const EnvStepLaunch& e);
// launch_thaw_frozen: chained rollouts under auto-reset - envs left frozen by an earlier rollout start their next episode
// (sample_initial_state with the env's episode counter + policy state reset, a bank's env to ITS policy's initial state), as the
// fused kernel's prologue does.  In place: state == next_state.
hipError_t launch_thaw_frozen(hipStream_t s, const EnvStepLaunch& e);
// rq_policy_bank_reset: hidden [16][ld] <- the initial state of every column's policy (weights [P][RQ_POLICY_NUM_WEIGHTS], block_policy
// [ld / 64])
hipError_t launch_bank_initial_hidden(hipStream_t s, uint32_t ld, float* hidden, const float* weights, const uint32_t* block_policy);
// chained mode of a tracked rollout, between the observation's assembly (k_observe, or the k_step before) and the actor: the row of
// each env's episode step count comes off obs [RQ_OBSERVATION_DIM][ld] in place, and the envs that are not frozen add this step's
// tracking error - the fused kernel's arithmetic (rq_device_math.hpp track_*).  Appends a graph node under a GraphSink.
hipError_t launch_track_shift(hipStream_t s, Batch b, const float* state, StatsPtrs st, float* obs, TrackPtrs trk);
// an env that carries a sensor schedule, behind whatever assembled its observation in obs [RQ_OBSERVATION_DIM][ld] (k_observe,
// or the k_step that folds the next one) and in front of launch_track_shift: the envs that are not frozen put columns 0..17 into the
// slot of their episode step count and take those of d' steps ago in their place (rq_device_math.hpp sensor_*; the fused kernel's
// functions).  Appends a graph node under a GraphSink.
hipError_t launch_sensor_apply(hipStream_t s, Batch b, StatsPtrs st, float* obs, SensorPtrs sn);
// chained mode: copy step t (env obs/action buffers + last reward / done code) into the trajectory
hipError_t launch_record(hipStream_t s, Batch b, const float* obs, const float* act, StatsPtrs st, TrajPtrs traj);
// ---- MFMA operand images of the policy (layout rationale: rq_device_math.hpp "actor") ----------
// lane l = (q = l >> 4, j = l & 15); one image = 64 dwords, one per lane.
// f32 actor (v_mfma_f32_16x16x4_f32): one float image per A operand / bias vector
enum {
    QW_L0 = 0,    //  6: layer_0, K-step s: lane (q,j) = W0[j][4s+q]; input 22 -> b0[j], input 23 -> 0
    QW_GI = 6,    // 12: W_input,  [m][s]: lane (q,j) = Wi[16m+j][4q+s]
    QW_GH = 18,   // 12: W_hidden, [m][s]: lane (q,j) = Wh[16m+j][4q+s]
    QW_L2 = 30,   // 16: layer_2 on the VALU, [r][i]: lane (q,j) = W2[i][4q+r] - the lane's slice of output row i
                  //     (round 3: the 16 quarter-filled MFMAs of layer_2 became 32 packed fmas on the Q layout + a
                  //     lane-group reduction through LDS, ActorF32T::layer2_*)
    // layer_0's bias rides in the spare K slot 22 (its B operand is the constant 1); the gate biases, pre-scaled,
    // enter through the C operand of each chain's first MFMA; layer_2's starts lane-group 0's partial sum
    QW_BR = 46,   //  4: [r]: -log2(e)  * (bi[4q+r] + bh[4q+r])
    QW_BZ = 50,   //  4: [r]: -log2(e)  * (bi[16+4q+r] + bh[16+4q+r])
    QW_BNI = 54,  //  4: [r]: -2log2(e) * bi[32+4q+r]
    QW_BNH = 58,  //  4: [r]: -2log2(e) * bh[32+4q+r]
    QW_H0 = 62,   //  4: [r]: initial_hidden_state[4q+r]
    QW_B2 = 66,   //  4: [i]: q == 0 ? b2[i] : 0   (addend of the lane-group's first partial product)
    QW_REGS = 70
};
// bf16 actor (v_mfma_f32_16x16x32_bf16): A operands are bf16x8 = 4 dword images each, element e of
// lane (q, i) in the low/high half of dword e/2; biases as in the f32 image
enum {
    BW_L0 = 0, BW_R = 4, BW_Z = 8, BW_NI = 12, BW_NH = 16, BW_L2 = 20,   // bf16x8 A operands, 4 dwords each
    BW_BR = 36, BW_BZ = 40, BW_BNI = 44, BW_BNH = 48, BW_H0 = 52, BW_B2 = 56,   // fp32, as in the f32 image
    BW_REGS = 60
};

// split-f16 actor (v_mfma_f32_16x16x32_f16, rq_device_math.hpp ActorF16X2): every A operand of the bf16 image twice,
// the f16 of the (gate-pre-scaled) weight and the f16 of its exact residual; biases fp32 as in the f32 image
enum {
    FW_L0H = 0, FW_L0L = 4, FW_RH = 8, FW_RL = 12, FW_ZH = 16, FW_ZL = 20, FW_NIH = 24, FW_NIL = 28, FW_NHH = 32,
    FW_NHL = 36, FW_L2H = 40, FW_L2L = 56,                                  // f16x8 A operands, 4 dwords each (layer_2: x 4 tiles)
    FW_BR = 72, FW_BZ = 76, FW_BNI = 80, FW_BNH = 84, FW_H0 = 88, FW_B2 = 92,   // fp32
    FW_REGS = 96
};

// Host-side packing of the 2 084 checkpoint parameters into the per-lane VGPR image the actor's
// v_mfma_f32_16x16x4_f32 instructions read as A / C operands (layout: rq_device_math.hpp "actor").
// the f32 image is stored in quads: images 4g .. 4g+3 of lane l at floats 256 g + 4 l .. + 3, one 16-byte load per lane
// and quad (qw_slot); the last quad is padded
enum { QW_QUADS = (QW_REGS + 3) / 4 };
constexpr int qw_slot(int v, int lane) { return (v >> 2) * 256 + lane * 4 + (v & 3); }
enum { RQ_PACKED_FLOATS = QW_QUADS * 256, RQ_PACKED_BF16_FLOATS = BW_REGS * 64, RQ_PACKED_F16X2_FLOATS = FW_REGS * 64 };
void pack_policy(const float* weights, float* packed);
// the same for the bf16 actor (v_mfma_f32_16x16x32_bf16): 36 dword images of bf16 pairs + 24 fp32 images
void pack_policy_bf16(const float* weights, float* packed);
// and for the split-f16 actor: 72 dword images of f16 pairs + 24 fp32 images
void pack_policy_f16x2(const float* weights, float* packed);
// the first weight whose pre-scaled operand has no f16 hi / lo split (magnitude >= 65 520), or -1 when the image holds them all
int policy_f16x2_misfit(const float* weights);
// The learner's transposed operands (rq_grad.hpp k_policy_grad_backward): unscaled weights, one 64-lane image per A operand.
// K-step (g, r) of a transposed gate product carries gate row 16 g + 4 q + r in k-slot q - the row the Q-layout delta holds
// in register r - so lane (q, j) = W[16 g + 4 q + r][j]; W2T: lane (q, j) = W2[q][j] (the 4 actions on K).
enum {
    GW_WIT = 0,   // 12: [g][r]: lane (q,j) = Wi[16g+4q+r][j]
    GW_WHT = 12,  // 12: [g][r]: lane (q,j) = Wh[16g+4q+r][j]
    GW_W2T = 24,  //  1: lane (q,j) = W2[q][j]
    GW_REGS = 25
};
enum { RQ_PACKED_GRAD_FLOATS = GW_REGS * 64 };
void pack_policy_grad(const float* weights, float* packed);
// both fp32 images as gather tables: pack_policy and pack_policy_grad themselves, run on symbols instead of numbers
// (table [RQ_PACKED_FLOATS] for the forward image, then [RQ_PACKED_GRAD_FLOATS] for the transposed one)
void pack_gather_table(PackGather* table);
// log-std rows of a SampleAndSquash head: w_ls [4][16] row-major (nullptr = zeros), b_ls [4] -> 20 x 64 floats
enum { RQ_LOGSTD_FLOATS = 20 * 64 };
void pack_logstd_head(const float* w_ls, const float* b_ls, float* image);

// ---- teacher bank (rq_teacher.hip): per-teacher operand images, regs x 64 lanes, one dword per lane --------
//   f32 : [H1/16][6] layer-1 A, [H2/16][H1/4] layer-2 A, [H2/4] layer-3 A, [H2/16][4] layer-2 bias, [4] layer-3 bias
//   bf16: the A operands as bf16x8 (4 dwords each): [H1/16], [H2/16][ceil(H1/32)], [ceil(H2/32)]; biases fp32 as above
constexpr int teacher_image_regs_f32(int h1, int h2) { return (h1 / 16) * 6 + (h2 / 16) * (h1 / 4) + h2 / 4 + (h2 / 16) * 4 + 4; }
constexpr int teacher_image_regs_bf16(int h1, int h2) {
    return 4 * (h1 / 16) + 4 * (h2 / 16) * ((h1 + 31) / 32) + 4 * ((h2 + 31) / 32) + (h2 / 16) * 4 + 4;
}
// split-f16 (v_mfma_f32_16x16x32_f16): every A operand of the bf16 image twice, hi then lo (f16 of the residual)
constexpr int teacher_image_regs_f16x2(int h1, int h2) {
    return 2 * (4 * (h1 / 16) + 4 * (h2 / 16) * ((h1 + 31) / 32) + 4 * ((h2 + 31) / 32)) + (h2 / 16) * 4 + 4;
}
// one teacher's parameters, [W1 (h1 x in) | b1 | W2 (h2 x h1) | b2 | W3 (4 x h2) | b3], rows = outputs -> its image
void pack_teacher_f32(const float* w, int in_dim, int h1, int h2, int act, int out_act, float* image);
void pack_teacher_bf16(const float* w, int in_dim, int h1, int h2, int act, int out_act, float* image);
// pack_teacher_f16x2 -> false when a pre-scaled weight lies outside the f16 range (|w| >= 65 520: its pieces would be +-inf)
bool pack_teacher_f16x2(const float* w, int in_dim, int h1, int h2, int act, int out_act, float* image);
// the generic dense stack (rq_teacher.hip k_teacher_relabel_layers): hidden layers padded to hp = 64 or 128 units, the fp32 image resident in LDS
// (layer 1 [6][hp/16][64] | per further hidden layer [hp/4][hp/16][64] + [hp] biases | output [hp/16][64][4] + [4] biases)
constexpr size_t teacher_layers_image_floats(int hp, int n_hidden) {
    return (size_t)6 * (hp / 16) * 64 + (size_t)(n_hidden - 1) * ((size_t)(hp / 4) * (hp / 16) * 64 + (size_t)hp) + (size_t)(hp / 16) * 64 * 4 + 4;
}
inline size_t teacher_layers_param_count(int in_dim, int n_hidden, const uint32_t* widths) {
    size_t n = 0;
    int prev = in_dim;
    for (int l = 0; l < n_hidden; ++l) { n += (size_t)widths[l] * prev + widths[l]; prev = (int)widths[l]; }
    return n + (size_t)4 * prev + 4;
}
// one teacher's parameters [W1 | b1 | ... | W_out | b_out] (rows = outputs) -> its streamed image
void pack_teacher_layers(const float* w, int in_dim, int n_hidden, const uint32_t* widths, int hp, int act, int out_act, float* image);
// teacher_start [n_teachers + 1] into sorted_env [n_envs] (the envs grouped by teacher): a column of a teacher = one (env, step) pair
hipError_t launch_teacher_relabel_layers(hipStream_t s, uint32_t n_teachers, uint32_t n_envs, uint32_t ld, uint32_t steps, uint32_t in_dim,
                                         uint32_t n_hidden, uint32_t hp, int act, int out_act, const float* images,
                                         const uint32_t* teacher_start, const uint32_t* sorted_env, const float* obs, float* actions);
inline size_t teacher_param_count(int in_dim, int h1, int h2) {
    return (size_t)h1 * in_dim + h1 + (size_t)h2 * h1 + h2 + (size_t)4 * h2 + 4;
}
// actions of every tile's teacher on the recorded observations obs [steps][22][ld] -> act [steps][4][ld];
// tile_teacher [n_tiles], tile_env [n_tiles][16] (0xFFFFFFFF = padding), images = bank in the given precision
hipError_t launch_teacher_relabel(hipStream_t s, uint32_t n_tiles, uint32_t ld, uint32_t steps, uint32_t in_dim,
                                  uint32_t h1, uint32_t h2, int act, int out_act, int precision, const float* images,
                                  const uint32_t* tile_teacher, const uint32_t* tile_env, const float* obs,
                                  float* actions);

// a teacher bank flying its envs (rq_teacher_rollout.hip k_rollout_teachers, the register-stationary fp32 family): the loop body
// README.md:95-99 x n_steps with env i driven by the teacher of its tile; tiles as launch_teacher_relabel's.  traj.obs == nullptr:
// no recording.  noise / autoreset: wave-uniform switches (0 / 1).  trk.ref != nullptr: on a moving setpoint (a fourth wave-uniform
// switch), a single table or a reference bank's per-env tables (TrackPtrs::row0_at).
struct TeacherRolloutArgs {
    Batch b; StepCfg c; NoiseCfg nc; SampleCfg sc; uint64_t seed; uint32_t epoch0, n_steps;
    uint32_t noise, autoreset;
    const float* params; float* state; StatsPtrs st; TrajPtrs traj;
    uint32_t in_dim; const float* images; const uint32_t* tile_teacher; const uint32_t* tile_env;
    TrackPtrs trk;
};
hipError_t launch_rollout_teachers(hipStream_t s, uint32_t n_tiles, uint32_t h1, uint32_t h2, int act, int out_act,
                                   const TeacherRolloutArgs& a);

// A fused rollout - the loop body README.md:95-99 x n_steps in one launch - of a policy or a policy bank, described once: what any of
// the kernel families (rq_fused_route.hpp) takes.  Set the fields by name; what a rollout does not use keeps its default.
struct FusedArgs {
    Batch b{}; StepCfg c{}; NoiseCfg nc{}; SampleCfg sc{}; uint64_t seed = 0; uint32_t epoch0 = 0, n_steps = 0;
    bool noise = false, autoreset = false;
    const float* params = nullptr; float* state = nullptr; float* hidden = nullptr;
    const float* weights = nullptr;                // raw weights (a bank: [P][RQ_POLICY_NUM_WEIGHTS]): the policy-state reset reads them
    StatsPtrs st{};
    TrajPtrs traj{};                               // obs != nullptr: recorded
    TrackPtrs trk{};                               // ref != nullptr: on a moving setpoint
    WrenchPtrs wr{};                               // rows != nullptr: the env's wrench schedule (fp32, no SampleAndSquash stage)
    VehiclePtrs vh{};                              // rows != nullptr: the env's vehicle schedule (fp32, no stage, no wrench schedule)
    WindPtrs wd{};                                 // rows != nullptr: the env's wind schedule (fp32, no stage, no other schedule)
    DelayPtrs dl{};                                // rows != nullptr: the env's delay schedule (fp32, no stage, no other schedule)
    SensorPtrs sn{};                               // rows != nullptr: the env's sensor schedule (fp32, no stage, no other schedule)
    // The actor.  One policy (block_policy == nullptr): `images` is its operand image in `precision`, with its output stage and its
    // native interval.  A policy bank (fp32, no output stage): the tables described above - `interval` is not read - and whether an
    // entry of policy_interval is above 1 (the host's knowledge: the table is on the device).
    int precision = RQ_POLICY_FP32;
    const float* images = nullptr; const uint32_t* block_policy = nullptr; const uint32_t* policy_interval = nullptr;
    SasArgs sas{};                                 // mode != RQ_SAS_OFF: only one policy, untracked, at interval 1
    uint32_t interval = 1;
    bool bank_rated = false;
    // != nullptr: every wave leaves (in, out | xcd << 60, loop begin, loop end) wall-clock ticks at span[4 * workgroup] and, behind
    // all of those, the core-clock cycles its steps took at span[4 * workgroups + workgroup] (rq_device_last_rollout_ms).  Round 2
    // took the kernel's begin / end from hipExtLaunchKernel events; calibrated under rocprofv3 in one process, an event-carrying
    // launch itself runs ~4 us longer than a plain one and the events read ~4 us more on top.
    unsigned long long* span = nullptr;
};
inline FusedTraits fused_traits(const FusedArgs& a) {
    return {a.b.n, a.precision, a.sas.mode != RQ_SAS_OFF, a.trk.ref != nullptr, a.wr.rows != nullptr, a.interval,
            a.block_policy != nullptr, a.bank_rated, a.vh.rows != nullptr, a.wd.rows != nullptr, a.dl.rows != nullptr,
            a.sn.rows != nullptr};
}
// The kernel route_fused(fused_traits(a)) names, enqueued on s; hipErrorInvalidValue, and nothing launched, for a description no
// kernel is built for.  n == 0 or n_steps == 0: nothing to do.
hipError_t launch_rollout_fused(hipStream_t s, const FusedArgs& a);
// layout changes at the boundary (device pointers): field-major [dim][ld] <-> row-major [n][dim|stride],
// dim <= 32; rows_to_soa zeroes the padding lanes n..ld-1
// slabs > 1: consecutive [dim][ld] blocks (the steps of a trajectory) -> consecutive [n][dim] blocks, one launch
hipError_t launch_soa_to_rows(hipStream_t s, const float* soa, uint32_t ld, uint32_t dim, uint32_t n, float* rows,
                              uint32_t slabs = 1);
hipError_t launch_rows_to_soa(hipStream_t s, const float* rows, uint32_t stride, uint32_t dim, uint32_t n, uint32_t ld,
                              float* soa);

// out[i] = value for i < count (uint32 / float / uint8 fills on the stream)
hipError_t launch_fill_f32(hipStream_t s, float* p, float v, uint32_t count);

}  // namespace rq
