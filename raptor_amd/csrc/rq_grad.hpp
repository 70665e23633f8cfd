// rq_grad.hpp — the learner half of distillation (README.md:208-216): the fp32 student's actions over a recorded trajectory and
// their exact gradient with respect to the 2 084 parameters, back through time along the recorded episode structure.
//
//   kernel                    what                                                           bound
//   k_policy_grad_forward     k_actor_relabel's pass + the state entering every step saved   f32 MFMA rate (+ 64 B/env-step stored)
//   k_policy_grad_backward    t = T-1 .. 0: recompute, W2^T / Wi^T / Wh^T da, outer products  f32 MFMA rate (+ 168 B/env-step read)
//   k_policy_grad_reduce      per-wave partials [waves][2084] -> [2084] in wave order         HBM (8 KB per wave)
// The distillation update (the masked MSE against a target, Adam, the operand images) without leaving the device:
//   k_policy_grad_forward_state   the forward without the action store (the saved state is all the seeded backward reads)
//   k_policy_loss_backward        the backward seeded by the loss itself: a = W2 h' + b2 recomputed with the forward's layer_2
//                                 arithmetic, dL/da = a - y on live entries; + per wave the squared error and the live count
//   k_policy_loss_reduce          partials in wave order, x 2 / M once; loss = SSE / M
//   k_adam_repack                 one workgroup: Adam on the 2 084 master weights, then both operand images from a gather table
// The same update for a bank of P policies, one per 64-env block (rq_grad_bank.hpp):
//   k_policy_grad_forward_state_bank   k_policy_grad_forward_state with the wave's image picked by block_policy[blockIdx.x]
//   k_policy_loss_backward_bank        k_policy_loss_backward likewise, both images
//   k_policy_loss_reduce_bank          per policy: its waves' partials in ascending wave order (a CSR list), x 2 / M_p; loss_p
//   k_adam_repack_bank                 one workgroup per policy: k_adam_repack on slot p; a policy without a wave is skipped whole
//   k_adam_set_lr_bank                 [P] learning rates in stream order
// The same two updates with a weight per env, or per env and step, in the loss (hold-out masks, teacher quality, emphasis by episode age):
//   k_policy_loss_backward_weighted[_bank]   dL/da = w (a - y) where the entry is live and w > 0; + per wave the weighted squared
//                                            error and, in float64, the sum of the counting weights
//   k_policy_loss_reduce_weighted[_bank]     the reductions above with W4 = that sum over the waves, in wave order, in M's place
// How well the student imitates, per env and bucket of episode age, from the forward alone:
//   k_policy_error_table[_bank]   the forward storing nothing of the pass: the lane sums its env's squared error (a - y)^2 over the
//                                 four actions per age bucket, sse / count [n_buckets][ld_out]; launch_policy_error_table
// What the policy does with what it knows, the effective feedback gains per env and bucket of episode age:
//   k_policy_gain_table[_bank]    the backward's recompute walked forwards, four local seeds e_i through W2 and Wi^T: the lane sums
//                                 A = da/dp0 [4][16] per age bucket, sum [n_buckets][4][16][ld_out]; launch_policy_gain_table
// The forwards, the backwards, the gain table, the loss reductions and the Adam kernels are one text each (rq_grad_forward.inc,
// rq_grad_backward.inc, rq_gain_table.inc, rq_loss_reduce.inc, rq_adam_repack.inc), compiled once per kernel.  Every form of the loss launch goes through one launcher,
// launch_policy_loss_grad (rq_grad_bank.hpp), from one description (rq_loss_launch.hpp).
//
// Layouts (rq_device_math.hpp "actor"): a wave owns 64 envs as 4 tiles of 16; lane (q, j) = (l >> 4, l & 15) holds, in the Q
// layout, rows 4q .. 4q+3 of a 16-vector of env (tile t, j).  What the reverse pass needs where:
//   * transposed products (feature on M, env on N, K = the vector being contracted): the delta in the Q layout is directly the B
//     operand (K-step r carries row 4q + r in k-slot q) and the transposed image (rq_pack.cpp pack_policy_grad) is the A operand;
//     the result is again in the Q layout - the reverse recurrence never changes layout;
//   * weight-gradient outer products (K = envs): both operands need feature j on lane j and env on k-slot q.  Every vector a
//     tile contributes goes through one 16-env x 156-float LDS tile per wave (row = env, one ds_write per value, read back
//     column-wise: k-step u takes envs 4u .. 4u+3), the way the observation already changes layout in the forward;
//   * the observation is read straight from the trajectory's field-major block in the B layout (feature 4s+q of env (t, j)),
//     the same floats k_actor_relabel's LDS trip gives its MFMAs; layer_0's bias rides on the constant-1 feature 22.
// Gate biases and the initial state's gradient are sums of deltas over envs: lane-local sums in the Q layout, folded over the 16
// lanes of a lane group in a fixed order at the end.  Nothing is accumulated with atomics: the result is the same bits every run.
// Device code, compiled as part of rq_kernels.hip (the library keeps one code object per kernel source).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rq_rollout.hpp"      // the actors, field(), kFusedBlock, WavesPerSimd
#include "rq_probe.hpp"        // ProbeEdges, kProbeMaxBuckets: the error table's age buckets are the probe's

namespace rq {

// ------------------------------------------------------------------ forward ------------
// k_actor_relabel (rq_kernels.hip) with one addition, the state entering step t in the Q layout to saved [t][16][ld] (every lane
// of the wave, padding included: the backward reads whole tiles), and two differences: the first state is the policy's (loaded)
// or the learned initial one, and nothing is written back to the policy.  The step is the actor's own: the actions are
// rq_trajectory_relabel's bit for bit.
#define RQ_GRAD_FORWARD_KERNEL k_policy_grad_forward
#define RQ_GRAD_STORE_ACT 1
#define RQ_GRAD_BANK 0
#include "rq_grad_forward.inc"

// the same pass without the action store: the saved state is all the loss-seeded backward reads
#define RQ_GRAD_FORWARD_KERNEL k_policy_grad_forward_state
#define RQ_GRAD_STORE_ACT 0
#define RQ_GRAD_BANK 0
#include "rq_grad_forward.inc"

// the same pass storing nothing of it: the squared imitation error against a target, per env and bucket of episode age, summed in
// the lane (rq_grad_forward.inc, RQ_GRAD_ERROR_TABLE) - 16 B/env-step of target read in place of 80 B/env-step of stores
#define RQ_GRAD_FORWARD_KERNEL k_policy_error_table
#define RQ_GRAD_STORE_ACT 0
#define RQ_GRAD_BANK 0
#define RQ_GRAD_ERROR_TABLE 1
#include "rq_grad_forward.inc"

// ------------------------------------------------------------------ backward -----------
// The LDS tile of the outer products: row = env of the tile, columns = the deltas (A operands) and inputs (B operands).
enum {
    GL_DR = 0, GL_DZ = 16, GL_DNI = 32, GL_DNH = 48, GL_D0 = 64,     // dL/d pre-activation: r, z, n (input half), n (hidden half), layer_0
    GL_DA = 80,                                                       // dL/da (4)
    GL_Y0 = 84, GL_HP = 100, GL_HN = 116, GL_X = 132,                 // layer_0 output, state before and after, observation (24)
    GL_ROW = 157                                                      // 156 used; odd: a column read touches 16 distinct banks
};
enum { GRAD_LANE_SUMS = 21 };      // per lane: r, z, n-input, n-hidden bias rows (4 each), h0 rows (4), b2 (1)

__device__ __forceinline__ float sigm2(float x) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x)); }

// One wave = 64 envs for the whole trajectory, walked backwards.  Per step and tile the forward step is recomputed from the saved
// state and the recorded observation with the forward's own MFMA chains and gate arithmetic (gru_gates_prescaled, element by
// element), so r, z, n and h' are the values the actions were computed from.  dc[t] = dL/d(state after the step) of tile t.
#define RQ_GRAD_BACKWARD_KERNEL k_policy_grad_backward
#define RQ_GRAD_SEEDED 0
#define RQ_GRAD_BANK 0
#include "rq_grad_backward.inc"

// the backward seeded by the loss itself (rq_grad_backward.inc)
#define RQ_GRAD_BACKWARD_KERNEL k_policy_loss_backward
#define RQ_GRAD_SEEDED 1
#define RQ_GRAD_BANK 0
#include "rq_grad_backward.inc"

// the same with a weight per env, or per env and step, on every entry of the loss (rq_grad_backward.inc, RQ_GRAD_WEIGHTED)
#define RQ_GRAD_BACKWARD_KERNEL k_policy_loss_backward_weighted
#define RQ_GRAD_SEEDED 1
#define RQ_GRAD_BANK 0
#define RQ_GRAD_WEIGHTED 1
#include "rq_grad_backward.inc"

// the backward's recompute walked forwards with four local seeds and no weight gradient: da/dp0 per env and bucket of episode age,
// summed in the lane (rq_gain_table.inc) - nothing of the recording's Jacobians is stored
#define RQ_GAIN_TABLE_KERNEL k_policy_gain_table
#define RQ_GRAD_BANK 0
#include "rq_gain_table.inc"

// grad[p] = sum over waves w = 0, 1, ... of partial[w][p], in that order
__global__ __launch_bounds__(256) void k_policy_grad_reduce(uint32_t waves, const float* __restrict__ partial,
                                                            float* __restrict__ grad) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= RQ_POLICY_NUM_WEIGHTS) return;
    float acc = 0.0f;
#pragma unroll 8
    for (uint32_t w = 0; w < waves; ++w) acc += partial[(size_t)w * RQ_POLICY_NUM_WEIGHTS + p];
    grad[p] = acc;
}

// The seeded backward's reduction (rq_loss_reduce.inc): the partials in wave order as k_policy_grad_reduce sums them, x 2 / M once;
// out[0] = loss, live_out[0] = M
#define RQ_LOSS_REDUCE_KERNEL k_policy_loss_reduce
#define RQ_GRAD_BANK 0
#include "rq_loss_reduce.inc"

// the same with W4, the waves' float64 weight sums, in M's place (rq_loss_reduce.inc, RQ_GRAD_WEIGHTED)
#define RQ_LOSS_REDUCE_KERNEL k_policy_loss_reduce_weighted
#define RQ_GRAD_BANK 0
#define RQ_GRAD_WEIGHTED 1
#include "rq_loss_reduce.inc"

// Adam on the master weights, then both operand images from a gather table: one workgroup (rq_adam_repack.inc)
#define RQ_ADAM_KERNEL k_adam_repack
#define RQ_GRAD_BANK 0
#include "rq_adam_repack.inc"

__global__ void k_adam_set_lr(AdamState* st, double lr) {
    if (threadIdx.x == 0 && blockIdx.x == 0) st->lr = lr;
}

// hidden [rows][ld] <- src[row]: the policy's reset when the initial state is known on the device only (after an update there)
__global__ __launch_bounds__(256) void k_fill_rows(float* __restrict__ dst, uint32_t ld, const float* __restrict__ src, uint32_t rows) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < ld)
        for (uint32_t r = 0; r < rows; ++r) dst[(size_t)r * ld + i] = src[r];
}

hipError_t launch_policy_grad_forward(hipStream_t s, uint32_t n, uint32_t ld, uint32_t steps, const float* packed,
                                      const float* obs, const uint8_t* done, const float* hidden, uint32_t ld_h,
                                      int start_initial, float* act, uint32_t ld_act, float* saved) {
    if (n == 0 || steps == 0) return hipSuccess;
    const unsigned g = (n + kFusedBlock - 1) / kFusedBlock;
    const uint32_t si = start_initial ? 1u : 0u;
    if (n > kOneWavePerSimdEnvs)        // launch_actor_relabel's choice of build (the two give the same bits)
        k_policy_grad_forward<ActorF32Lean><<<g, kFusedBlock, 0, s>>>(n, ld, steps, packed, obs, done, hidden, ld_h, si, act, ld_act, saved);
    else
        k_policy_grad_forward<ActorF32><<<g, kFusedBlock, 0, s>>>(n, ld, steps, packed, obs, done, hidden, ld_h, si, act, ld_act, saved);
    return hipGetLastError();
}

hipError_t launch_policy_grad_backward(hipStream_t s, uint32_t n, uint32_t ld, uint32_t steps, const float* packed,
                                       const float* gpacked, const float* obs, const uint8_t* done, const float* saved,
                                       const float* grad_act, uint32_t ld_g, int start_initial, float* grad_h_start,
                                       float* partial, float* grad) {
    if (n == 0 || steps == 0) return hipSuccess;
    const uint32_t waves = (n + 63) / 64;
    k_policy_grad_backward<<<waves, 64, 0, s>>>(n, ld, steps, packed, gpacked, obs, done, saved, grad_act, ld_g,
                                                start_initial ? 1u : 0u, grad_h_start, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_policy_grad_reduce<<<(RQ_POLICY_NUM_WEIGHTS + 255) / 256, 256, 0, s>>>(waves, partial, grad);
    return hipGetLastError();
}

hipError_t launch_adam_repack(hipStream_t s, const float* grad, float* w, float* m, float* v, AdamState* st, const PackGather* table,
                              float* packed, float* gpacked) {
    k_adam_repack<<<1, 1024, 0, s>>>(grad, w, m, v, st, table, (uint32_t)RQ_PACKED_FLOATS, (uint32_t)RQ_PACKED_GRAD_FLOATS, packed,
                                     gpacked);
    return hipGetLastError();
}

hipError_t launch_adam_set_lr(hipStream_t s, AdamState* st, double lr) {
    k_adam_set_lr<<<1, 64, 0, s>>>(st, lr);
    return hipGetLastError();
}

hipError_t launch_fill_rows(hipStream_t s, float* dst, uint32_t ld, const float* src, uint32_t rows) {
    if (ld == 0 || rows == 0) return hipSuccess;
    k_fill_rows<<<(ld + 255) / 256, 256, 0, s>>>(dst, ld, src, rows);
    return hipGetLastError();
}

}  // namespace rq
