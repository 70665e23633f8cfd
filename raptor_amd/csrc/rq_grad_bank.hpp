// rq_grad_bank.hpp - the distillation update of rq_grad.hpp for a bank of P policies, one per 64-env block (rq_rollout_policies'
// granularity): a sweep of learning rates or seeds costs one student's launch count.
//
//   kernel                             what                                                              grid
//   k_policy_grad_forward_state_bank   k_policy_grad_forward_state, the wave's image picked per block      waves
//   k_policy_loss_backward_bank        k_policy_loss_backward, both images picked per block                waves
//   k_policy_loss_reduce_bank          policy p: its waves' partials in ascending wave order, x 2 / M_p    (ceil(2084 / 256), P)
//   k_policy_loss_backward_weighted_bank   k_policy_loss_backward_weighted, both images picked per block   waves
//   k_policy_loss_reduce_weighted_bank     policy p: as above with W4_p, its waves' float64 weight sums    (ceil(2084 / 256), P)
//   k_adam_repack_bank                 k_adam_repack on slot p; a policy that owns no wave is skipped       P
//   k_adam_set_lr_bank                 up to 256 learning rates, carried as kernel arguments                1
//   k_policy_error_table_bank          k_policy_error_table, the wave's image picked per block             waves
//   k_policy_gain_table_bank           k_policy_gain_table, both images picked per block                   waves
// The weights are wave-uniform MFMA operands read once from an image pointer, so the seeded pair is the single policy's text
// (rq_grad_forward.inc, rq_grad_backward.inc under RQ_GRAD_BANK) with that pointer chosen by block_policy[blockIdx.x], as
// k_rollout_fused_bank chooses it: a wave computes what it computes for a policy of its own, bit for bit.  The reduction is the single
// policy's, segmented: a policy's waves come from a CSR list (wave_offsets [P + 1] into wave_list [waves], ascending within a
// policy), so its gradient and loss are those of a recording that holds its blocks only, in order.  The reductions and the Adam kernels
// are the single policy's texts too (rq_loss_reduce.inc, rq_adam_repack.inc under RQ_GRAD_BANK).
// launch_policy_loss_grad, the one launcher of every loss launch (rq_loss_launch.hpp), is here, below all the kernels it picks from.
// Device code, compiled as part of rq_kernels.hip.
#pragma once
#include "rq_grad.hpp"

namespace rq {

#define RQ_GRAD_FORWARD_KERNEL k_policy_grad_forward_state_bank
#define RQ_GRAD_STORE_ACT 0
#define RQ_GRAD_BANK 1
#include "rq_grad_forward.inc"

// k_policy_error_table with the wave's image picked per block (rq_grad_forward.inc under RQ_GRAD_BANK and RQ_GRAD_ERROR_TABLE)
#define RQ_GRAD_FORWARD_KERNEL k_policy_error_table_bank
#define RQ_GRAD_STORE_ACT 0
#define RQ_GRAD_BANK 1
#define RQ_GRAD_ERROR_TABLE 1
#include "rq_grad_forward.inc"

#define RQ_GRAD_BACKWARD_KERNEL k_policy_loss_backward_bank
#define RQ_GRAD_SEEDED 1
#define RQ_GRAD_BANK 1
#include "rq_grad_backward.inc"

#define RQ_GRAD_BACKWARD_KERNEL k_policy_loss_backward_weighted_bank
#define RQ_GRAD_SEEDED 1
#define RQ_GRAD_BANK 1
#define RQ_GRAD_WEIGHTED 1
#include "rq_grad_backward.inc"

// k_policy_gain_table with both of the wave's images picked per block (rq_gain_table.inc under RQ_GRAD_BANK)
#define RQ_GAIN_TABLE_KERNEL k_policy_gain_table_bank
#define RQ_GRAD_BANK 1
#include "rq_gain_table.inc"

// k_policy_loss_reduce per policy (blockIdx.y), segmented by the CSR list (rq_loss_reduce.inc under RQ_GRAD_BANK)
#define RQ_LOSS_REDUCE_KERNEL k_policy_loss_reduce_bank
#define RQ_GRAD_BANK 1
#include "rq_loss_reduce.inc"

// k_policy_loss_reduce_weighted per policy likewise: W4_p over p's waves
#define RQ_LOSS_REDUCE_KERNEL k_policy_loss_reduce_weighted_bank
#define RQ_GRAD_BANK 1
#define RQ_GRAD_WEIGHTED 1
#include "rq_loss_reduce.inc"

// k_adam_repack, workgroup p on slot p; a policy that owns no wave is skipped whole (rq_adam_repack.inc under RQ_GRAD_BANK)
#define RQ_ADAM_KERNEL k_adam_repack_bank
#define RQ_GRAD_BANK 1
#include "rq_adam_repack.inc"

// st [first + i].lr = rates.lr [i * stride] for i < count <= 256 (stride 0: one rate for all).  The rates travel as kernel arguments:
// a call takes effect in stream order, and the caller's array is its own again when the launch returns.
struct AdamLrChunk { double lr[256]; };
__global__ __launch_bounds__(256) void k_adam_set_lr_bank(AdamState* __restrict__ st, uint32_t first, uint32_t count, uint32_t stride,
                                                          AdamLrChunk rates) {
    const uint32_t i = threadIdx.x;
    if (i < count) st[first + i].lr = rates.lr[i * stride];
}

// the forward of a loss launch in the build `Actor`
template <typename Actor>
static hipError_t launch_loss_forward(hipStream_t s, const LossLaunch& a) {
    const unsigned g = (a.n + kFusedBlock - 1) / kFusedBlock;
    const uint32_t si = a.start_initial ? 1u : 0u;
    if (a.block_policy)
        k_policy_grad_forward_state_bank<Actor><<<g, kFusedBlock, 0, s>>>(a.n, a.ld, a.steps, a.packed, a.block_policy, (uint32_t)RQ_PACKED_FLOATS,
                                                                          a.obs, a.done, a.hidden, a.ld_h, si, a.saved);
    else
        k_policy_grad_forward_state<Actor><<<g, kFusedBlock, 0, s>>>(a.n, a.ld, a.steps, a.packed, a.obs, a.done, a.hidden, a.ld_h, si, a.saved);
    return hipGetLastError();
}

// The first launch of a loss launch alone: the forward that saves the state and stores no action (the probes read nothing else).
hipError_t launch_policy_grad_forward_state(hipStream_t s, const LossLaunch& a) {
    if (a.n == 0 || a.steps == 0 || (a.block_policy && a.n_policies == 0)) return hipErrorInvalidValue;
    // launch_policy_grad_forward's choice of build (the two give the same bits)
    return a.n > kOneWavePerSimdEnvs ? launch_loss_forward<ActorF32Lean>(s, a) : launch_loss_forward<ActorF32>(s, a);
}

// Every form of the loss launch (rq_loss_launch.hpp): three launches, the backward and the reduction picked by (bank, weighted).
hipError_t launch_policy_loss_grad(hipStream_t s, const LossLaunch& a) {
    const bool bank = a.block_policy != nullptr, weighted = a.weight != nullptr;
    if (weighted && (a.ld_w < a.n || (a.weight_steps != 1 && a.weight_steps != a.steps))) return hipErrorInvalidValue;
    hipError_t e = launch_policy_grad_forward_state(s, a);
    if (e != hipSuccess) return e;
    const LossPartialLayout lay = loss_partial_layout(a.n, weighted);
    const uint32_t si = a.start_initial ? 1u : 0u, w_step = a.weight_steps == 1 ? 0u : a.ld_w;
    const uint32_t fl = RQ_PACKED_FLOATS, gfl = RQ_PACKED_GRAD_FLOATS;
    float* const partial = a.partial + lay.partial;
    float* const wave_sse = a.partial + lay.sse;
    double* const wave_wsum = reinterpret_cast<double*>(a.partial + lay.wsum);
    uint32_t* const wave_live = reinterpret_cast<uint32_t*>(a.partial + lay.live);
    const dim3 rgrid((RQ_POLICY_NUM_WEIGHTS + 255) / 256, bank ? a.n_policies : 1u);
    if (bank && weighted)
        k_policy_loss_backward_weighted_bank<<<lay.waves, 64, 0, s>>>(a.n, a.ld, a.steps, a.packed, a.gpacked, a.block_policy, fl, gfl, a.obs,
                                                                      a.done, a.saved, a.target, a.ld_y, a.weight, a.ld_w, w_step, si, partial,
                                                                      wave_sse, wave_wsum);
    else if (bank)
        k_policy_loss_backward_bank<<<lay.waves, 64, 0, s>>>(a.n, a.ld, a.steps, a.packed, a.gpacked, a.block_policy, fl, gfl, a.obs, a.done,
                                                             a.saved, a.target, a.ld_y, si, partial, wave_sse, wave_live);
    else if (weighted)
        k_policy_loss_backward_weighted<<<lay.waves, 64, 0, s>>>(a.n, a.ld, a.steps, a.packed, a.gpacked, a.obs, a.done, a.saved, a.target,
                                                                 a.ld_y, a.weight, a.ld_w, w_step, si, partial, wave_sse, wave_wsum);
    else
        k_policy_loss_backward<<<lay.waves, 64, 0, s>>>(a.n, a.ld, a.steps, a.packed, a.gpacked, a.obs, a.done, a.saved, a.target, a.ld_y, si,
                                                        partial, wave_sse, wave_live);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (bank && weighted)
        k_policy_loss_reduce_weighted_bank<<<rgrid, 256, 0, s>>>(a.wave_offsets, a.wave_list, partial, wave_sse, wave_wsum, a.grad, a.loss);
    else if (bank)
        k_policy_loss_reduce_bank<<<rgrid, 256, 0, s>>>(a.wave_offsets, a.wave_list, partial, wave_sse, wave_live, a.grad, a.loss);
    else if (weighted)
        k_policy_loss_reduce_weighted<<<rgrid, 256, 0, s>>>(lay.waves, partial, wave_sse, wave_wsum, a.grad, a.loss);
    else
        k_policy_loss_reduce<<<rgrid, 256, 0, s>>>(lay.waves, partial, wave_sse, wave_live, a.grad, a.loss, a.live);
    return hipGetLastError();
}

// the error table of a launch in the build `Actor`: the single kernel or the bank's, picked here and nowhere else
template <typename Actor>
static hipError_t launch_error_table(hipStream_t s, const ErrorTableLaunch& a, const ProbeEdges& edges) {
    const LossLaunch& p = a.pass;
    const unsigned g = (p.n + kFusedBlock - 1) / kFusedBlock;
    const uint32_t si = p.start_initial ? 1u : 0u;
    if (p.block_policy)
        k_policy_error_table_bank<Actor><<<g, kFusedBlock, 0, s>>>(p.n, p.ld, p.steps, p.packed, p.block_policy, (uint32_t)RQ_PACKED_FLOATS, p.obs,
                                                                   p.done, p.hidden, p.ld_h, si, p.target, p.ld_y, edges, a.n_buckets, a.sse,
                                                                   a.count, a.ld_out);
    else
        k_policy_error_table<Actor><<<g, kFusedBlock, 0, s>>>(p.n, p.ld, p.steps, p.packed, p.obs, p.done, p.hidden, p.ld_h, si, p.target, p.ld_y,
                                                              edges, a.n_buckets, a.sse, a.count, a.ld_out);
    return hipGetLastError();
}

// The error table (rq_loss_launch.hpp ErrorTableLaunch): one launch, the forward's choice of build.  A description whose strides or
// buckets would let a lane read or write beside its column is refused here, whatever the caller checked.
hipError_t launch_policy_error_table(hipStream_t s, const ErrorTableLaunch& a) {
    static_assert(kErrorTableMaxBuckets == kProbeMaxBuckets, "the error table's buckets are the probe's");
    const LossLaunch& p = a.pass;
    if (p.n == 0 || p.steps == 0 || (p.block_policy && p.n_policies == 0)) return hipErrorInvalidValue;
    if (a.n_buckets < 1 || a.n_buckets > kErrorTableMaxBuckets || a.ld_out < p.n || p.ld_y < p.n || p.ld < p.n) return hipErrorInvalidValue;
    if (!p.packed || !p.obs || !p.done || !p.target || !a.sse || !a.count || (!p.start_initial && !p.hidden)) return hipErrorInvalidValue;
    ProbeEdges edges{};
    for (uint32_t b = 0; b <= a.n_buckets; ++b) {
        if (b > 0 && a.edges[b] <= a.edges[b - 1]) return hipErrorInvalidValue;
        edges.v[b] = a.edges[b];
    }
    return p.n > kOneWavePerSimdEnvs ? launch_error_table<ActorF32Lean>(s, a, edges) : launch_error_table<ActorF32>(s, a, edges);
}

// The gain table (rq_loss_launch.hpp GainTableLaunch): one launch, one wave per 64-env block, the single kernel or the bank's picked
// here and nowhere else.  A description whose strides or buckets would let a lane read or write beside its cells is refused here,
// whatever the caller checked.
hipError_t launch_policy_gain_table(hipStream_t s, const GainTableLaunch& a) {
    const LossLaunch& p = a.pass;
    if (p.n == 0 || p.steps == 0 || (p.block_policy && p.n_policies == 0)) return hipErrorInvalidValue;
    if (a.n_buckets < 1 || a.n_buckets > kErrorTableMaxBuckets || a.ld_out < p.n || p.ld < p.n) return hipErrorInvalidValue;
    if (!p.packed || !p.gpacked || !p.obs || !p.done || !a.sum || !a.count || (!p.start_initial && (!p.hidden || p.ld_h < p.n)))
        return hipErrorInvalidValue;
    ProbeEdges edges{};
    for (uint32_t b = 0; b <= a.n_buckets; ++b) {
        if (b > 0 && a.edges[b] <= a.edges[b - 1]) return hipErrorInvalidValue;
        edges.v[b] = a.edges[b];
    }
    const uint32_t waves = (p.n + 63) / 64, si = p.start_initial ? 1u : 0u;
    if (p.block_policy)
        k_policy_gain_table_bank<<<waves, 64, 0, s>>>(p.n, p.ld, p.steps, p.packed, p.gpacked, p.block_policy, (uint32_t)RQ_PACKED_FLOATS,
                                                      (uint32_t)RQ_PACKED_GRAD_FLOATS, p.obs, p.done, p.hidden, p.ld_h, si, edges, a.n_buckets,
                                                      a.sum, a.count, a.ld_out);
    else
        k_policy_gain_table<<<waves, 64, 0, s>>>(p.n, p.ld, p.steps, p.packed, p.gpacked, p.obs, p.done, p.hidden, p.ld_h, si, edges,
                                                 a.n_buckets, a.sum, a.count, a.ld_out);
    return hipGetLastError();
}

hipError_t launch_adam_repack_bank(hipStream_t s, uint32_t n_policies, const uint32_t* wave_offsets, const float* grad, float* w, float* m,
                                   float* v, AdamState* st, const PackGather* table, float* images, float* gimages) {
    if (n_policies == 0) return hipErrorInvalidValue;
    k_adam_repack_bank<<<n_policies, 1024, 0, s>>>(wave_offsets, grad, w, m, v, st, table, (uint32_t)RQ_PACKED_FLOATS,
                                                   (uint32_t)RQ_PACKED_GRAD_FLOATS, images, gimages);
    return hipGetLastError();
}

hipError_t launch_adam_set_lr_bank(hipStream_t s, AdamState* st, uint32_t n_policies, const double* lr, uint32_t n_lr) {
    if (n_lr != 1 && n_lr != n_policies) return hipErrorInvalidValue;
    AdamLrChunk c{};
    for (uint32_t first = 0; first < n_policies; first += 256) {
        const uint32_t count = n_policies - first < 256u ? n_policies - first : 256u;
        if (n_lr == 1) c.lr[0] = lr[0];
        else for (uint32_t i = 0; i < count; ++i) c.lr[i] = lr[first + i];
        k_adam_set_lr_bank<<<1, 256, 0, s>>>(st, first, count, n_lr == 1 ? 0u : 1u, c);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace rq
